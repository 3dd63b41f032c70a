/*
 * rovat.h — C ABI of librovat_hip.so, the MI355X-native batched rigid-body
 * backend behind RoboVat's `env.step()` hot path.
 *
 * This header is the drop-in boundary.  Each entry point
 * replaces the reference-side interface cited next to it (file:line relative
 * to the StanfordVL/robovat tree).  Everything is `extern "C"`, plain pointers
 * and sizes; no torch / HIP types appear in the signatures (a HIP stream is
 * passed as `void*`).  Bulk buffers named `d_*` are DEVICE pointers, buffers
 * named `h_*` are HOST pointers.  The caller owns every buffer it passes in;
 * the library never frees caller memory.
 *
 * Conventions (must match robovat/math, third_party/transformations.py:1034-1359):
 *   quaternions are xyzw, Euler angles are static-xyz ("sxyz"), poses are
 *   world-frame, SI units, float32 everywhere on the device.
 *
 * Error convention (reference: Python exceptions, bullet_physics.py:162,184,
 * 779,1286): every call returns an int status, 0 = RV_OK; rv_last_error()
 * returns a thread-local message.  The Python shim maps codes to the same
 * exception types the reference raises.
 */
#ifndef ROVAT_H_
#define ROVAT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- compile-time capacities (one env = one wave64; state lives in LDS) ---- */
#define RV_MAXB        4   /* max movable bodies per env (MAX_MOVABLE_BODIES)      */
#define RV_MAXH        4   /* convex hulls per shape (V-HACD parts)                */
#define RV_MAXV       16   /* vertices per convex hull                             */
#define RV_MAXP       28   /* faces per convex hull (2 V - 4 for V = 16)           */
#define RV_PC_MAXPIX 2048  /* visible pixels of one body kept for point-cloud sampling (more: every stride-th one, or this many evenly spaced if num_points needs them) */
#define RV_MAX_SHAPES 16   /* shape templates per scene                            */
#define RV_NJ          9   /* arm joints: 7 limb (right_j0..j6) + 2 finger         */
#define RV_NLIMB       7
#define RV_NFRAME     10   /* link frames: 7 limb links, hand, l_finger, r_finger  */
#define RV_NCOL       10   /* arm collider boxes                                   */
#define RV_MAXTILES   24   /* tiles per list of a push layout (layouts.py:25-245)  */
#define RV_MAXG        4   /* NUM_GOAL_STEPS upper bound (push_env.py:72)          */
#define RV_MAXQ        8   /* link-target pose queue (controllable_body.py:133)    */
#define RV_NBB   (RV_MAXB * (RV_MAXB - 1) / 2)
#define RV_NMAN  (2 * RV_MAXB + RV_NBB) /* manifolds: body-table, body-body, arm-body */
#define RV_BODY_STRIDE 13  /* pos3, quat4(xyzw), lin3, ang3                        */

/* status codes -> Python exceptions in robovat_amd/lib.py */
#define RV_OK            0
#define RV_ERR_VALUE     1   /* ValueError   */
#define RV_ERR_STATE     2   /* RuntimeError */
#define RV_ERR_HIP       3   /* RuntimeError (HIP runtime failure) */
#define RV_ERR_NOTIMPL   4   /* NotImplementedError */

/* task ids (push_reward.py:282-299) */
#define RV_TASK_NONE      0
#define RV_TASK_CLEARING  1
#define RV_TASK_INSERTION 2
#define RV_TASK_CROSSING  3

#define RV_ENV_PUSH  0
#define RV_ENV_GRASP 1
/* phases of Grasp4DofEnv._execute_action (grasp_4dof_env.py:300-308) */
#define RV_GPHASE_INITIAL  0
#define RV_GPHASE_OVERHEAD 1
#define RV_GPHASE_PRESTART 2
#define RV_GPHASE_START    3
#define RV_GPHASE_END      4
#define RV_GPHASE_POSTEND  5
#define RV_GPHASE_DONE     6
/* phases of PushEnv._execute_action (push_env.py:121-127) */
#define RV_PHASE_INITIAL  0
#define RV_PHASE_PRE      1
#define RV_PHASE_START    2
#define RV_PHASE_MOTION   3
#define RV_PHASE_POST     4
#define RV_PHASE_OFFSTAGE 5
#define RV_PHASE_DONE     6

/* One convex-decomposed shape template, expressed in its centre-of-mass /
 * principal-axes frame at unit scale (replaces URDF+OBJ ingest,
 * bullet_physics.py:143-186; hull format of tools/convert_obj_to_urdf.py). */
typedef struct rv_shape {
  int32_t n_hulls;
  int32_t n_verts[RV_MAXH];
  float   verts[RV_MAXH][RV_MAXV][3];
  float   inertia_k[3]; /* principal inertia per unit mass at unit scale        */
  float   radius;       /* bounding radius about the COM at unit scale          */
  /* face planes n.x <= d of every hull (same frame, unit scale), for the depth /
   * segmentation render behind SegmentedPointCloudObs (bullet_camera.py:188-235) */
  int32_t n_planes[RV_MAXH];
  float   planes[RV_MAXH][RV_MAXP][4];
} rv_shape;

/* Kinematic description of the Sawyer-like arm (replaces the URDF tree that
 * sawyer_sim.py:86-171 loads; numbers are BUILD-CHOSEN). */
typedef struct rv_arm {
  float base_pos[3];
  float base_quat[4];
  float jpos[RV_NLIMB + 1][3];   /* parent->child origin; entry 7 = fixed hand frame */
  float jquat[RV_NLIMB + 1][4];
  float q_lo[RV_NJ], q_hi[RV_NJ];
  float v_max[RV_NJ];            /* URDF velocity limits (joint.py:57)          */
  float a_max[RV_NJ];            /* effort-equivalent acceleration limits       */
  float finger_y0[2];            /* finger frame y offset in the hand frame     */
  int32_t col_frame[RV_NCOL];    /* which link frame each collider box rides on */
  float col_center[RV_NCOL][3];
  float col_half[RV_NCOL][3];
  /* 1 / (URDF effort limit) of every joint (1 / N m; fingers 1 / N), 0 = unlimited.  PyBullet's
   * POSITION_CONTROL motors are limited to the joint effort (bullet_physics.py:1061-1104: default
   * max force); with the kinematic limb the limit acts on what the arm can push with: the normal
   * impulse of an arm - body contact row is capped at dt x min_j tau_j / |J_j . n| over the joints
   * upstream of the collider (rv_config.arm_effort_limit) */
  float inv_tau_max[RV_NJ];
  /* inertial parameters of the limb (URDF <inertial>; controllable_body.py:458-466 drives PyBullet's
   * btMultiBody, which has them from the URDF): link i rides on frame i (i < 7), entry 7 = the hand
   * with the gripper; mass, centre of mass in the frame, principal moments (taken diagonal in the
   * frame).  Read by rv_config.limb_dynamics only */
  float link_mass[RV_NLIMB + 1];
  float link_com[RV_NLIMB + 1][3];
  float link_inertia[RV_NLIMB + 1][3];
} rv_arm;

typedef struct rv_scene {
  int32_t  n_shapes;
  rv_shape shapes[RV_MAX_SHAPES];
  rv_arm   arm;
} rv_scene;

/* Every config key the hot path reads, flattened.
 * Values are BUILD-CHOSEN defaults in robovat_amd/configs.py because the
 * reference's YAML files are not distributed with its source. */
typedef struct rv_config {
  /* world */
  int32_t  n_envs;
  int32_t  env_id_offset;        /* global id of env 0 on this rank            */
  uint32_t seed_lo, seed_hi;
  float    dt;                   /* simulator.py:26                            */
  float    gravity_z;            /* simulator.py:27                            */
  /* contact solver.  breaking: Bullet's gContactBreakingThreshold, a FACTOR -- the threshold of a
   * manifold is breaking x the smaller angular-motion disc of its two shapes (bounding radius of
   * a movable, half diagonal of a collider box; btCollisionShape::getContactBreakingThreshold) */
  int32_t  solver_iters;
  float    erp, slop, margin, breaking, warmstart, max_pushout;
  float    lin_damp, ang_damp;   /* per-substep velocity multipliers           */
  float    contact_query_dist;   /* check_contact threshold (simulator.py:246) */
  float    solver_tol;           /* PGS stops when max |d lambda| < tol (0 = run all iterations) */
  /* body deactivation ("sleeping", Bullet default behaviour): a body whose
   * speeds stay below the thresholds for sleep_steps substeps is put to
   * sleep until something comes near it (0 steps = never sleep) */
  float    sleep_lin, sleep_ang;
  int32_t  sleep_steps;
  /* a body that only oscillates in place (rocking on an edge) is at rest too: it
   * also goes to sleep when its pose stayed within sleep_pos_win metres and
   * sleep_rot_win (largest quaternion component change) of where it was when the
   * window opened, for sleep_steps substeps (0 = velocity test only) */
  float    sleep_pos_win, sleep_rot_win;
  /* narrow-phase gating: a pair's full GJK/feature pass is re-run only after
   * its bodies moved np_gate metres (linear + angular*radius) since the last
   * pass, when a cached point was lost, or every np_max_age-th substep; cached
   * points are refreshed every substep (np_max_age = 0: every substep) */
  float    np_gate;
  int32_t  np_max_age;
  /* table (arm_env.py:78-99; layouts.py:30) */
  float    table_center[2];
  float    table_half[2];
  float    table_thickness;
  float    table_z;
  float    table_height_range[2];
  float    table_friction;
  float    arm_friction;
  float    fall_depth;           /* bodies this far below the table are frozen */
  /* movable bodies (push_env.py:399-597) */
  int32_t  n_bodies_min, n_bodies_max;
  float    scale_range[2], mass_range[2], friction_range[2];
  float    margin_xy;
  float    pose_lo[6], pose_hi[6];
  float    drop_mass, drop_friction;
  float    safe_drop_height;
  int32_t  n_movable_shapes;
  int32_t  movable_shapes[RV_MAX_SHAPES];
  int32_t  n_target_shapes;
  int32_t  target_shapes[RV_MAX_SHAPES];
  /* layout (layouts.py:14-24) */
  int32_t  task;
  int32_t  layout_id;
  int32_t  use_tiles;
  float    tile_size;
  float    tile_offset[2];
  int32_t  n_region, n_goal, n_target, n_obstacle;
  float    region[RV_MAXTILES][2];
  float    goal[RV_MAXTILES][2];
  float    target[RV_MAXTILES][2];
  float    obstacle[RV_MAXTILES][2];
  /* arm control (controllable_body.py:14-25; sawyer_sim.py:186-308) */
  float    kp, kd;
  float    velocity_threshold;
  float    limb_max_velocity_ratio;
  float    limb_timeout;
  float    limb_position_threshold;
  int32_t  ik_iters;
  float    ik_damping, ik_residual, ik_max_step;
  float    neutral_positions[RV_NLIMB];
  float    offstage_positions[RV_NLIMB];
  int32_t  open_gripper_when_reset;
  /* push env (push_env.py:58-94, 631-937) */
  float    cspace_low[3], cspace_high[3];
  float    translation_x, translation_y;
  float    finger_tip_offset;
  float    gripper_safe_height;
  float    min_delta_position, min_delta_angle;
  float    workspace_x_range, workspace_y_range;
  int32_t  steps_check, max_phase_steps, max_motion_steps, max_offstage_steps;
  int32_t  num_goal_steps;       /* 0 = None                                   */
  int32_t  max_steps;            /* 0 = None (robot_env.py:214)                */
  float    success_thresh;
  /* observation (camera_obs.py:127-238): SegmentedPointCloudObs over the simulated
   * Kinect2 depth camera (push_env.py:50-55; bullet_camera.py:18-23).  Extrinsics as in
   * the reference: x_cam = cam_rotation * x_world + cam_translation (camera.py:76-79),
   * intrinsics fx, fy, cx, cy, skew (bullet_camera.py:47-51). */
  int32_t  num_points;
  int32_t  cam_height, cam_width;
  float    cam_intrinsics[5];
  float    cam_rotation[9];
  float    cam_translation[3];
  float    cam_near;
  int32_t  use_crop;             /* OBS.CROP_MIN / CROP_MAX (camera_obs.py:187-192)  */
  float    crop_min[3], crop_max[3];
  /* Grasp4DofEnv (grasp_4dof_env.py:63-345) and the force-limited gripper it needs */
  int32_t  env_type;             /* RV_ENV_PUSH / RV_ENV_GRASP                        */
  int32_t  finger_dynamics;      /* 1: the two finger joints are dynamic DOFs of the
                                  * contact solver, driven by POSITION_CONTROL motor rows
                                  * limited to finger_max_force (bullet_physics.py:1061-1104:
                                  * default max force = joint effort)                 */
  float    finger_mass, finger_max_force;
  float    grasp_cuboid_low[3], grasp_cuboid_high[3];   /* ACTION.CUBOID (:144-150)   */
  float    overhead_positions[RV_NLIMB];                /* ARM.OVERHEAD_POSITIONS     */
  int32_t  max_action_steps;                            /* SIM.MAX_ACTION_STEPS (:333)*/
  float    end_effector_step;                           /* sawyer_sim.py:264          */
  /* lateral friction the env gives the finger tips / the table while it descends and
   * while it lifts (grasp_4dof_env.py:262-270, 282-293)                              */
  float    grasp_mu_descend[2], grasp_mu_lift[2];
  /* the ground the table stands on (arm_env.py:85-88): a body that leaves the table lands on
   * it; below ground_z - fall_depth a body is frozen (safety net) */
  float    ground_z, ground_friction;
  /* rolling / spinning friction of a body on its support (urdf_template.xml:11-16: 0.001;
   * Body.set_dynamics passes spinning = rolling, body.py:229): a resisting angular impulse of at
   * most rolling_friction x (normal impulse of the body - table manifold) per substep */
  float    rolling_friction;
  /* a sleeping body is woken by the moving arm when a collider box comes within wake_gap of its
   * hulls (contact imminent); min(breaking threshold of the pair, wake_gap) is used.  Contact points of an AWAKE body
   * are still created at the contact-breaking distance; at larger gaps they carry no impulse, so
   * waking later changes the work, not the motion */
  float    wake_gap;
  /* Bullet's own deactivation rule (btRigidBody::updateDeactivation, gDeactivationTime): a body
   * slower than deact_lin / deact_ang for deact_steps substeps in a row that touches nothing awake
   * but the table goes to sleep as well (0 steps: rule off) */
  float    deact_lin, deact_ang;
  int32_t  deact_steps;
  /* horizontal components of the gravity vector (simulator.py:27 takes a 3-vector;
   * bullet_physics.py:129-137 set_gravity); gravity_z above is the third */
  float    gravity_xy[2];
  /* 1: arm - body contact forces are limited by the joint efforts (rv_arm.inv_tau_max) */
  int32_t  arm_effort_limit;
  /* 1: the seven limb joints are dynamic while the arm touches a body (SURVEY.md 8 f1;
   * controllable_body.py:458-466, bullet_physics.py:1061-1104): the solver of such a substep has the
   * joint velocities as unknowns next to the body velocities -- joint-space inertia M(q) of the chain
   * (composite bodies, rv_arm.link_*), contact rows with their joint-space Jacobians, and one
   * POSITION_CONTROL motor row per joint that pulls the joint back to the commanded velocity with at most
   * the joint effort (1 / rv_arm.inv_tau_max) minus what the free motion and holding the arm against
   * gravity already take.  A pad that lands on an object then stalls instead of crushing it.  0: the
   * limb is a kinematic pusher (its trajectory does not depend on contacts) */
  int32_t  limb_dynamics;
  /* > 0: an island also stops when its residual has not fallen below the smallest one seen so far for this
   * many sweeps in a row -- a Gauss-Seidel that cycles (friction rows dithering at the cone under a body the
   * arm pins to the table) instead of converging; 0: only solver_tol / solver_iters end a solve */
  int32_t  solver_stall;
  /* > 0: an island all of whose bodies were below the sleep thresholds (sleep_lin / sleep_ang) after the last
   * substep sweeps until its residual is below solver_tol_rest instead of solver_tol.  (With the plain 1e-5 N s
   * exit resting bodies creep at ~4e-5 m/s -- visible only without deactivation; Bullet runs its 50 sweeps without
   * an early exit.)  Islands that hold finger / limb motor rows keep solver_tol.  0 (or >= solver_tol): one tolerance */
  float    solver_tol_rest;
  /* ArmEnv._reset_camera (arm_env.py:109-152; push_env.py:273-280): on every env.reset() the camera of that env gets the
   * calibration above plus uniform noise in [-cam_noise, +cam_noise], element by element: [0..4] the five intrinsics
   * (fx, fy, cx, cy, skew), [5..13] the rotation matrix, [14..16] the translation (KINECT2.DEPTH.*_NOISE; 0 = none) */
  float    cam_noise[17];
  /* ArmEnv._reset_scene (arm_env.py:94-99): `if SIM.WALL.USE: self.wall = simulator.add_body(SIM.WALL.PATH, SIM.WALL.POSE,
   * is_static=True)`.  wall_use = 1: every env.reset() puts a STATIC body (mass 0: it collides with the movable bodies and
   * is seen by the cameras, nothing moves it) of shape template wall_shape, scaled by wall_scale, at wall_pose (x, y, z,
   * quaternion) into body slot RV_MAXB - 1; n_bodies_max must then leave that slot free.  0: no wall */
  int32_t  wall_use, wall_shape;
  float    wall_scale;
  float    wall_pose[7];
} rv_config;

/* Per-launch statistics of rv_step_macro / rv_reset (device-side reductions of
 * the counters push_env.py:136-141,729-733 keeps). */
typedef struct rv_macro_stats {
  int64_t substeps;      /* sum over envs of Simulator.step() calls           */
  int64_t env_steps;     /* envs that completed an env.step()                 */
  int64_t unsafe, ineffective, useful, successes, episodes_done;
  int64_t max_substeps;  /* slowest env of the launch                         */
  int64_t awake_substeps;/* substeps in which at least one body was awake     */
} rv_macro_stats;

typedef struct rv_world rv_world;

/* ---- lifecycle: Simulator.__init__/reset/start (simulator.py:23-92),
 *      BulletPhysics.__init__/reset/start (bullet_physics.py:31-104) ---- */
int  rv_create(const rv_config* cfg, const rv_scene* scene, int device, rv_world** out);
int  rv_destroy(rv_world* w);
const char* rv_last_error(void);
int  rv_set_stream(rv_world* w, void* hip_stream);
int  rv_synchronize(rv_world* w);
int  rv_num_envs(const rv_world* w);
/* which build of the env kernel this world launches (chosen once, in rv_create): RV_ENV_BUILD_OCC1 = k_env (all
 * registers, one wave per SIMD), RV_ENV_BUILD_OCC2 = k_env_occ2 (256 registers, two waves per SIMD); 0 for NULL */
#define RV_ENV_BUILD_OCC1 1
#define RV_ENV_BUILD_OCC2 2
int  rv_env_kernel_build(const rv_world* w);

/* ---- RobotEnv.reset (robot_env.py:204-237) = PushEnv._reset_scene +
 *      _load_movable_bodies + _sample_body_poses(_on_tiles) (push_env.py:331-597)
 *      + ArmEnv._reset_robot (arm_env.py:101-107).  d_env_mask: uint8[N], NULL = all. */
int  rv_reset(rv_world* w, const uint8_t* d_env_mask);

/* ---- RobotEnv.step (robot_env.py:239-275) = PushEnv._execute_action
 *      (push_env.py:631-733) + get_observation + get_reward, for all envs whose
 *      episode is not done.  d_actions: float[N][G][4] in [-1,1]. ---- */
int  rv_set_actions(rv_world* w, const float* d_actions);
int  rv_step_macro(rv_world* w);

/* ---- generate_episode's inner loop (episode_generation.py:44-46) for the
 *      on-device RandomPolicy: n_steps x { action = policy(obs); env.step(action) }
 *      per env inside ONE launch, so an env never waits for the slowest env of
 *      the batch between steps.  Actions are the rv_policy_random() draws for
 *      macro indices first_macro_index .. +n_steps-1; with auto_reset != 0 an
 *      env whose episode ended is reset (as rv_reset would) before its next
 *      step, otherwise it stops.  d_rewards / d_dones: optional [n_steps][N]. */
int  rv_rollout(rv_world* w, int32_t n_steps, int32_t first_macro_index, int32_t auto_reset,
                float* d_rewards, uint8_t* d_dones);
/* Partial batches (EnvPool style), for policies that run on the host and must not wait for the
 * slowest env of every batched env.step() (robot_env.py:239-275; the reference's worker
 * processes are just as independent, tools/parallel_run.py:54-90).  rv_step_begin gives the envs
 * flagged in d_mask (NULL: all) their next action ([N][G][4]); rv_step_poll advances every env
 * that is in the middle of a step by at most max_substeps Simulator.step() calls (one more when a coasting run of the
 * arm ends on the budget: the regular substep it stopped at is still taken) and / or about
 * max_usec microseconds of GPU time (0 = no limit) and sets d_finished[i] = 1 for the envs whose
 * env.step() completed in this launch; for those envs -- and only those -- row i of the optional
 * obs / d_reward / d_done ([N] rows, as rv_observe / rv_reward lay them out) receives what
 * env.step() returned (rows of the other envs are unspecified; their point-cloud rows are
 * zeroed).  An env.step() may take several polls; WHAT an env computes does not depend
 * on how its step is cut into launches: its trajectory is rv_step_macro's, bit for bit.  A step
 * begun on an env whose episode is over is reported finished at once (reward 0, done).
 * Mixing with the lock-step entry points: rv_step_macro, rv_rollout*, rv_step_sub and
 * rv_wait_until_stable CANCEL the pending partial step of every env they run on (the env is no
 * longer "stepping": a later poll does not resume or repeat it; the physics the cancelled step
 * already did stays done); rv_reset cancels it as well.  Begin a new step to continue.
 * Both env types: PushEnv (push_env.py:631-733) and Grasp4DofEnv (grasp_4dof_env.py:213-293: its phase loop ticks after
 * every substep; the reward's wait_until_stable is resumable like the closing wait of a push). */
int  rv_step_begin(rv_world* w, const float* d_actions /* [N][G][4] */, const uint8_t* d_mask /* [N] or NULL */);
/* on != 0: a step begun on an env whose episode is over RESETS it instead (RobotEnv.reset, robot_env.py:204-237,
 * as the loop of generate_episodes does between episodes, episode_generation.py:36-46): the next poll reports the
 * env finished with what env.reset() returns -- its observation, reward 0, done 0 -- and the action is not taken.
 * The reset is not cut by the poll's budget (a poll that resets envs lasts as long as their drop-and-settle).
 * Default: off (the env is reported finished at once with reward 0, done). */
int  rv_set_auto_reset(rv_world* w, int32_t on);
struct rv_obs_buffers;
int  rv_step_poll(rv_world* w, int32_t max_substeps, int32_t max_usec, uint8_t* d_finished /* [N] */,
                  const struct rv_obs_buffers* obs /* or NULL */, float* d_reward /* [N] or NULL */, uint8_t* d_done /* [N] or NULL */);
/* The same rollout returning what every env.step() of the loop returns
 * (robot_env.py:275: observation, reward, done): per-step observation rows
 * [n_steps][N]... in the layouts of rv_obs_buffers (NULL members are skipped;
 * steps not taken are zero rows).  The segmented point clouds of all steps are
 * rendered from per-step pose snapshots right after the stepping kernel. */
int  rv_rollout_record(rv_world* w, int32_t n_steps, int32_t first_macro_index, int32_t auto_reset,
                       float* d_rewards, uint8_t* d_dones, const struct rv_obs_buffers* step_obs /* host struct of device pointers */);
/* ---- the same loop run the way the reference runs it at scale: every env is an
 *      independent worker (tools/parallel_run.py:54-90 starts one process per
 *      env, none waits for another).  The N envs share a pool of
 *      total_env_steps env.step() calls; each env takes its next step (auto-reset
 *      when its episode ended) while the pool lasts.  The k-th step an env takes
 *      uses macro index first_macro_index + k, so every env's trajectory is the
 *      prefix of the rv_rollout trajectory of the same length.
 *      d_steps_taken: optional [N], the number of steps each env took. ---- */
int  rv_rollout_async(rv_world* w, int32_t total_env_steps, int32_t first_macro_index, int32_t* d_steps_taken);

/* ---- RandomPolicy._action (random_policy.py:14-23): U(-1,1)^(G*4) from
 *      Philox keyed by (seed, global env id, macro_index). ---- */
int  rv_policy_random(rv_world* w, int32_t macro_index, float* d_actions);
/* ---- HeuristicPushPolicy._action / HeuristicPushSampler._sample
 *      (push_policy.py:33-52, heuristic_push_sampler.py:66-123). ---- */
int  rv_policy_heuristic(rv_world* w, int32_t max_attempts, float* d_actions);

/* ---- AntipodalGrasp4DofPolicy._action (grasp_policy.py:17-75) over
 *      AntipodalDepthImageGraspSampler._sample(depth, intrinsics, 1)
 *      (image_grasp_sampler.py:149-375), one grasp per env; the semantics and
 *      the departures are written out in csrc/rv_dev_grasp_sampler.h. ---- */
#define RV_AP_MAX_RADIUS  32    /* Gaussian radius int(4 sigma + 0.5) <= 32 (sigma < 7.875) */
#define RV_AP_MAX_EDGES 4096    /* edge pixels one env may have (LDS: 12 B each)            */
#define RV_AP_OK              1 /* status per env: a grasp                                  */
#define RV_AP_NO_EDGES        0 /*   no edge pixel                                          */
#define RV_AP_NO_PAIRS      (-1)/*   no valid (antipodal, narrow enough) pair               */
#define RV_AP_ALL_REJECTED  (-2)/*   'Failed to sample any valid grasp.' (:359-360)          */
#define RV_AP_TOO_MANY_EDGES (-3)/*  more than RV_AP_MAX_EDGES edge pixels (never truncated) */
typedef struct rv_antipodal_params {
  /* config.SAMPLER (grasp_policy.py:30-46) */
  float   friction_coef;               /* FRICTION_COEF                                      */
  float   depth_grad_thresh;           /* DEPTH_GRAD_THRESH                                  */
  float   depth_grad_gaussian_sigma;   /* DEPTH_GRAD_GAUSSIAN_SIGMA                          */
  int32_t downsample_rate;             /* DOWNSAMPLE_RATE, 1..8                              */
  int32_t max_rejection_samples;       /* MAX_REJECTION_SAMPLES, >= 1                        */
  int32_t use_crop;                    /* 0: CROP = None (the whole image)                   */
  int32_t crop[4];                     /* CROP = [r0, c0, r1, c1]                            */
  float   min_dist_from_boundary;      /* MIN_DIST_FROM_BOUNDARY > max(WH, WW)               */
  float   min_grasp_dist;              /* MIN_GRASP_DIST (rv_policy_antipodal_multi only)      */
  float   angle_dist_weight;           /* ANGLE_DIST_WEIGHT (unused: _sample never passes it)  */
  int32_t depth_samples_per_grasp;     /* DEPTH_SAMPLES_PER_GRASP, must be 1                 */
  float   min_depth_offset;            /* MIN_DEPTH_OFFSET                                   */
  float   max_depth_offset;            /* MAX_DEPTH_OFFSET                                   */
  float   depth_sample_window_height;  /* DEPTH_SAMPLE_WINDOW_HEIGHT (WH), >= 1              */
  float   depth_sample_window_width;   /* DEPTH_SAMPLE_WINDOW_WIDTH (WW), >= 1               */
  /* config.GRIPPER_WIDTH (grasp_policy.py:47), metres; <= 0: no width limit */
  float   gripper_width;
  /* computed on the host in float64 and rounded to float32 */
  float   cone_cos;                    /* cos(arctan(FRICTION_COEF))                         */
  int32_t gauss_radius;                /* int(4 sigma + 0.5), 0 when sigma <= 1e-15          */
  float   gauss_weights[RV_AP_MAX_RADIUS + 1]; /* w[k], k = 0..radius: exp(-k^2 / 2 sigma^2), normalised over -radius..radius */
} rv_antipodal_params;
/* d_depth: [N][H][W] eye-z depth (0 = nothing hit), NULL = rv_render it now.
 * d_image_grasps [N][5]: [x1, y1, x2, y2, depth] in image pixels.  d_actions4 [N][4] (or NULL): the grasp as
 * Grasp2D.from_vector(...).as_4dof() in the world with the env's own calibration (rv_get_camera).  d_status [N]:
 * RV_AP_*.  A row whose status is not RV_AP_OK carries the env's rv_policy_random draw for macro_index in
 * d_actions4, and in d_image_grasps that draw's centre projected through the env's camera, [u, v, u, v, z].
 * A grasp world only; invalid parameters: RV_ERR_VALUE. */
int  rv_policy_antipodal(rv_world* w, const float* d_depth, const rv_antipodal_params* h_params, int32_t macro_index,
                         float* d_image_grasps, float* d_actions4, int32_t* d_status);
/* ---- sample(depth, camera, num_samples) (image_grasp_sampler.py:220-375): up to num_samples DISTINCT grasps per env in
 *      one launch, the reference's walk (:303-375) over the same key order as rv_policy_antipodal: a pair is accepted
 *      when it passes the per-candidate checks and min_k image_dist(candidate, accepted_k) > MIN_GRASP_DIST, as NumPy
 *      evaluates it (a NaN distance accepts); the walk stops at num_samples grasps or after
 *      min(MAX_REJECTION_SAMPLES, #valid) pairs.  The weight of the angle term is image_dist's default 1.0:
 *      ANGLE_DIST_WEIGHT stays unused, as in the reference.  d_image_grasps [N][K][5], d_actions4 [N][K][4] (or NULL),
 *      K = num_samples; d_count [N]: the grasps found; rows count..K-1 repeat row 0 (grasps[:, :] = grasp, :366).
 *      Row 0 is the grasp of rv_policy_antipodal, depth included; row k draws its depth from Philox counter words
 *      (0xffffffff, 0xffffffff - k).  d_status [N]: RV_AP_OK when count >= 1, else the codes above under their rules,
 *      and then all K rows carry the env's rv_policy_random draw and its projection.  RV_ERR_VALUE: whatever
 *      rv_policy_antipodal refuses, num_samples outside [1, RV_AP_MAX_SAMPLES], a NULL d_count. ---- */
#define RV_AP_MAX_SAMPLES 64
int  rv_policy_antipodal_multi(rv_world* w, const float* d_depth, const rv_antipodal_params* h_params, int32_t macro_index,
                               int32_t num_samples, float* d_image_grasps, float* d_actions4, int32_t* d_count, int32_t* d_status);
/* ---- grasp-centred depth crops: what a grasp-quality model reads for each candidate.  The reference's
 *      image_utils.transform (robovat/perception/image_utils.py:14-41: translate the grasp centre to the image centre,
 *      rotate the grasp axis onto the image's x axis about (W/2, H/2), nearest neighbour, zero outside) followed by
 *      image_utils.crop (:44-86) about the centre, for K image grasps per env in one launch.  With theta the angle of
 *      p2 - p1 and g the midpoint of row (n, k), the image of that row is
 *        crop(transform(depth[n], (H/2 - g_y, W/2 - g_x), theta), h*step, w*step)[step/2::step, step/2::step]
 *      (step 1: the reference's two calls) wherever the (h*step) x (w*step) window lies inside the image; an output
 *      pixel whose window position lies outside it is read from the source all the same (the reference composition
 *      gives 0 there).  The arithmetic -- float32, unfused, a source coordinate rounded by floor(v + 0.5), inside
 *      decided in float before any conversion -- is written out in csrc/rv_dev_grasp_sampler.h.  Agreement with
 *      OpenCV's warpAffine on pixels whose source coordinate lies at a rounding boundary is unverified.  A NaN,
 *      infinite or far-away row gives an all-zero image.  d_depth [N][H][W] (H, W from the params), d_grasps [N][K][5]
 *      as rv_policy_antipodal_multi writes them, d_images [N][K][h][w], d_grasp_depths [N][K] (or NULL): column 4 of the
 *      rows.  Any world, push or grasp: it supplies N, the device and the stream; no env is read or changed.
 *      Asynchronous on the world's stream.  RV_ERR_VALUE, with every output left untouched: a NULL pointer other than
 *      d_grasp_depths, a buffer that is not 4-byte aligned, height or width < 1, crop_height or crop_width outside
 *      [1, RV_GC_MAX_SIDE], step outside [1, RV_GC_MAX_STEP], k outside [1, RV_AP_MAX_SAMPLES]. ---- */
#define RV_GC_MAX_SIDE 256
#define RV_GC_MAX_STEP 16
typedef struct rv_grasp_crop_params {
  int32_t height, width;            /* of the depth images */
  int32_t crop_height, crop_width;  /* h, w of one output image, 1 .. RV_GC_MAX_SIDE */
  int32_t step;                     /* 1 .. RV_GC_MAX_STEP: every step-th pixel of an (h*step) x (w*step) crop */
  int32_t reserved[3];
} rv_grasp_crop_params;
int  rv_grasp_crops(rv_world* w, const rv_grasp_crop_params* h_params, const float* d_depth, const float* d_grasps, int32_t k,
                    float* d_images, float* d_grasp_depths);
/* ---- grasp-quality network: one logit per candidate from its crop (rv_grasp_crops) and its grasp depth, so that K
 *      candidates can be ranked without executing them.  It replaces the choice of the reference's
 *      AntipodalGrasp4DofPolicy (robovat/policies/grasp_policy.py:60-73), which takes sample(depth, intrinsics, 1) --
 *      the first candidate -- as it comes.  Fixed topology, sizes in the descriptor (BUILD-CHOSEN, the reference has no
 *      such model):
 *        a = (x - im_mean) * im_inv_std;  u = (z - z_mean) * z_inv_std
 *        c1 = pool2(relu(conv5x5_same(a; 1 -> c1)));  c2 = pool2(relu(conv3x3_same(c1; c1 -> c2)))
 *        f1 = relu(fc(flatten(c2) -> f1));  p = relu(fc(u -> p));  f2 = relu(fc(concat(f1, p) -> f2));  logit = fc(f2 -> 1)
 *      The output is the logit (no exponential on the device; a probability is sigmoid(logit)).  The arithmetic -- one
 *      float32 FMA chain per dot product, from the bias, in ascending input index -- and the layout of the weight blob
 *      are written out in csrc/rv_dev_grasp_quality.h.  Ranges: height and width multiples of 4 in
 *      [RV_GQ_MIN_SIDE, RV_GQ_MAX_SIDE]; c1 and c2 multiples of 4 in [4, RV_GQ_MAX_CHANNELS]; f1 and f2 multiples of 4 in
 *      [4, RV_GQ_MAX_FEATURES]; p a multiple of 4 in [4, RV_GQ_MAX_POSE]; reserved 0.  The default model is 32 x 32,
 *      c1 = c2 = 16, f1 = f2 = 64, p = 16 (73 617 floats); the smallest is 8 x 8 with 4 everywhere.
 *      rv_grasp_quality_weight_count: floats in the blob of such a model, or -1 for a NULL or refused descriptor.
 *      rv_grasp_quality: d_weights the blob, d_images [N][k][height][width], d_grasp_depths [N][k], d_logits [N][k].
 *      Stateless: any world, it supplies N, the device and the stream; no env is read or changed.  Asynchronous on the
 *      world's stream.  RV_ERR_VALUE before any launch, with d_logits left untouched: a NULL pointer, a buffer that is not
 *      4-byte aligned, a size outside its range, k outside [1, RV_AP_MAX_SAMPLES], a normalisation constant that is not
 *      finite. ---- */
#define RV_GQ_MIN_SIDE 8
#define RV_GQ_MAX_SIDE 32
#define RV_GQ_MAX_CHANNELS 16
#define RV_GQ_MAX_FEATURES 128
#define RV_GQ_MAX_POSE 32
typedef struct rv_grasp_quality_model { int32_t height, width, c1, c2, f1, f2, p, reserved;
                                        float im_mean, im_inv_std, z_mean, z_inv_std; } rv_grasp_quality_model;
int64_t rv_grasp_quality_weight_count(const rv_grasp_quality_model* h_model);
int  rv_grasp_quality(rv_world* w, const rv_grasp_quality_model* h_model, const float* d_weights,
                      const float* d_images, const float* d_grasp_depths, int32_t k, float* d_logits);
/* ---- a training step of that network on the device (csrc/rv_dev_grasp_train.h has it operation for operation;
 *      DESIGN.md §24).  The loss stays with the caller: the forward entry returns logits, the caller computes
 *      g[b] = dL/dlogit[b] (any loss; no exponential runs in a kernel) and hands it to the backward entry.  Unlike
 *      rv_grasp_quality the batch size m is a parameter, 1 .. RV_GQ_MAX_BATCH, not the world's N x k.
 *      rv_grasp_quality_train_workspace_floats: floats of workspace for m samples (about 57 KB per sample at the default
 *      sizes), or -1 for a NULL or refused descriptor or m outside its range.
 *      rv_grasp_quality_forward_train: d_logits [m] are rv_grasp_quality's logits of the same rows, bit for bit; the
 *      workspace keeps per sample the pooled c1 and c2, which position of its 2 x 2 window each pool chose (v00, then
 *      v01, v10, v11 each under a strict >: ties go to the first), f1, p, f2 and the normalised grasp depth.
 *      rv_grasp_quality_backward: d_grad [weight_count] in the blob's layout, every float written, from d_dlogits [m] and
 *      the workspace the forward entry filled for the SAME weights, images and depths.  Every gradient is a float32 chain
 *      from +0 whose order depends on the shapes alone (no atomics, no dependence on grid, tile or m's divisibility):
 *        relu passes where the stored activation is > 0; a pool window passes to its chosen position when the pooled
 *        value is > 0; what is not passed is +0.
 *        fc layers: the gradient at an input is the fma chain over the layer's outputs o ascending of (dy[o], W[o][i]);
 *        dW[o][i] is the fma chain over the samples b ascending of (dy[b][o], x[b][i]), db[o] the sum chain of dy[b][o].
 *        conv2 and conv1: per sample, s[co][ci][ky][kx] is the fma chain over the passing pool windows of channel co in
 *        row-major order of (dz, the zero-padded input at the chosen position shifted by the tap), the bias part the sum
 *        chain of dz over the same windows; dW and db are the sum chains of these over b ascending.  The gradient at c1
 *        is the fma chain over (co, ky, kx) ascending of the taps that land on a chosen position of a passing window.
 *        No gradient goes to the image or the grasp depth.
 *      rv_adam_step, per element: m' = fma(beta1, m, (1 - beta1) g); v' = fma(beta2, v, ((1 - beta2) g) g);
 *      w' = w - (lr (m' corr1)) / (sqrtf(v' corr2) + eps), every operation rounded on its own, sqrtf and / correctly;
 *      corr1 = 1 / (1 - beta1^t) and corr2 = 1 / (1 - beta2^t) are the caller's (float64, rounded once).
 *      All four are stateless like rv_grasp_quality: the world supplies the device and the stream, no env is read or
 *      written; asynchronous on the world's stream.  RV_ERR_VALUE before any launch, with every output untouched: a NULL
 *      pointer, a buffer that is not 4-byte aligned, a model rv_grasp_quality refuses, a normalisation constant that is
 *      not finite, m outside [1, RV_GQ_MAX_BATCH], d_grad overlapping an input or the workspace, the workspace, the
 *      logits and the weights overlapping one another, count < 1, Adam buffers that overlap, an Adam parameter that is
 *      not finite, a beta outside [0, 1), a nonzero reserved word. ---- */
#define RV_GQ_MAX_BATCH 4096
int64_t rv_grasp_quality_train_workspace_floats(const rv_grasp_quality_model* h_model, int64_t m);
int  rv_grasp_quality_forward_train(rv_world* w, const rv_grasp_quality_model* h_model, const float* d_weights,
                                    const float* d_images, const float* d_grasp_depths, int64_t m,
                                    float* d_workspace, float* d_logits);
int  rv_grasp_quality_backward(rv_world* w, const rv_grasp_quality_model* h_model, const float* d_weights,
                               const float* d_images, const float* d_grasp_depths, const float* d_dlogits, int64_t m,
                               float* d_workspace, float* d_grad);
typedef struct rv_adam_params { float lr, beta1, beta2, eps, corr1, corr2; int32_t reserved[2]; } rv_adam_params;
int  rv_adam_step(rv_world* w, const rv_adam_params* h_params, int64_t count, float* d_w, const float* d_g,
                  float* d_m, float* d_v);
/* ---- cross-entropy refinement of grasp candidates: the step between two scorings (score, keep the elites, resample
 *      around them, score again -- how a grasp-quality network is normally used; with try_grasps rewards as scores, an
 *      evolutionary search with the simulator as the model).  One launch per iteration; the arithmetic, operation for
 *      operation, is in csrc/rv_dev_grasp_refine.h.
 *      d_depth [N][H][W] (H, W from the params); d_grasps [N][k][5] as rv_policy_antipodal_multi or an earlier call of
 *      this function wrote them; d_scores [N][k] logits or rewards; d_count, d_status [N] the sampler's outputs, either
 *      may be NULL: input row j of env n is a CANDIDATE when (no d_status or status[n] == RV_AP_OK) and (no d_count or
 *      j < count[n]).  V = the env's candidates, ranked in the total order of rv_cem_refit (descending, the lower index
 *      first among equals, +0 == -0, NaNs last and by index); E' = min(n_elites, V).
 *      d_grasps_out [N][k][5] (must not be d_grasps): V = 0: the k rows copied bit for bit.  Otherwise rows 0 .. E'-1 are
 *      the elites in rank order, bit for bit (their crops and logits are the same next round: an env's best score never
 *      goes down), and row j >= E' is a child of elite r = (j - E') mod E', [x1, y1, x2, y2, z]: with g = 0.5 (p1 + p2),
 *      a = 0.5 (p2 - p1) and four standard normals z0 .. z3 (Box-Muller of rv_dev_cem.h, |z| <= 5.77) the child has
 *      centre g + sigma_center (z0, z1), half axis a rotated by sigma_angle z2, and depth z + sigma_depth z3 clamped to
 *      [cd + MIN_DEPTH_OFFSET, cd + MAX_DEPTH_OFFSET], cd the child's own centre-depth window minimum.  It is accepted
 *      when its centre (of the row as written) lies inside the crop, passes the sampler's step 8 on the unfiltered
 *      image (distance from the crop boundary >= MIN_DIST_FROM_BOUNDARY; cd neither 0 nor NaN) and its five floats are
 *      finite; else the row is its parent's, bit for bit.  Antipodality is not re-checked.
 *      d_parent [N][k] (or NULL): the input index of the parent for an elite and an accepted child, -1 - parent for a
 *      child that fell back; j itself where V = 0.  d_count_out [N] (or NULL): k where V > 0, else 0.
 *      d_actions4_out [N][k][4] (or NULL): ap_grasp_4dof of output row j with the env's own calibration, the conversion
 *      of rv_policy_antipodal_multi; it needs a grasp world.  Without it any world will do, as with rv_grasp_crops: it
 *      supplies N, the global env ids, the seed, the device and the stream.
 *      h_sampler supplies use_crop, crop, min_dist_from_boundary, depth_sample_window_height / _width, min_depth_offset
 *      and max_depth_offset, nothing else (but all of it is checked as rv_policy_antipodal_multi checks it).
 *      Draws: Philox keyed by the world's seed, the GLOBAL env id, macro_index in [0, 2^24), iteration in [0, 2^26), the
 *      params' seed, the output row and the component -- not by N, k or n_elites; a key space of its own.
 *      No env state is read beyond the id and the calibration, none is changed.  Asynchronous on the world's stream.
 *      RV_ERR_VALUE before any launch, with every output untouched: a NULL required pointer, a buffer that is not
 *      4-byte aligned, d_grasps_out == d_grasps, k outside [1, RV_AP_MAX_SAMPLES], n_elites outside [1, k], height or
 *      width < 1, a sigma that is negative or not finite, macro_index or iteration outside its range, a nonzero reserved
 *      word, sampler parameters that rv_policy_antipodal_multi would refuse, d_actions4_out on a push world. ---- */
typedef struct rv_grasp_refine_params {
  int32_t height, width;        /* of the depth images                                          */
  int32_t macro_index, iteration; /* Philox: the env.step() being chosen, the refinement round  */
  uint32_t seed;                /* the policy's seed, on top of the world's                     */
  int32_t n_elites;             /* E in [1, k]                                                  */
  float   sigma_center;         /* px,  >= 0, finite                                            */
  float   sigma_angle;          /* rad, >= 0, finite                                            */
  float   sigma_depth;          /* m,   >= 0, finite                                            */
  int32_t reserved[3];
} rv_grasp_refine_params;
int  rv_grasp_refine(rv_world* w, const rv_grasp_refine_params* h_params, const rv_antipodal_params* h_sampler,
                     const float* d_depth, const float* d_grasps, const float* d_scores, const int32_t* d_count,
                     const int32_t* d_status, int32_t k, float* d_grasps_out, float* d_actions4_out,
                     int32_t* d_parent, int32_t* d_count_out);

/* ---- planning-mode PushReward: get_reward_fn(task, layout, is_planning=True) (push_reward.py:272-374 with the
 *      planning branches :110-151 insertion_termination, :168-200 crossing_termination, :230-238 check_stride,
 *      :241-254 check_border, :257-269 check_target_border, :312-357), what a sampling-based planner scores the
 *      candidate transitions of its plans with.  States are the xy positions of B bodies, [..][B][2] float32; task,
 *      tile lists, tile size and offset are the world's rv_config (task, region, goal, n_region, n_goal, tile_size,
 *      tile_offset); RV_TASK_NONE gives reward 1, termination 0 (dummy_reward_fn, :34-47).  The semantics are written
 *      out in csrc/rv_dev_plan.h.  Neither call reads more of an env than its last observation, and neither changes
 *      any env state.  Asynchronous on the world's stream.  RV_ERR_VALUE: n_bodies outside 1..RV_MAXB, s < 1, h < 1,
 *      m < 0, a missing required pointer, a buffer that is not 8-byte aligned, a grasp world. ---- */
typedef struct rv_plan_params {
  int32_t n_bodies;          /* B, 1..RV_MAXB: bodies per state (the reference uses state.shape[1]) */
  int32_t is_high_level;     /* stride limits 0.1 / 0.3 instead of 0.01 / 0.15 (:313-322)           */
  int32_t use_dense_reward, use_time_penalty;
  float   goal_reward, termination_reward, dense_reward, time_reward;  /* 100, -100, 1, -1 (:274-277) */
  float   gamma;             /* discount of rv_plan_score; 1 = plain sum                            */
} rv_plan_params;
/* reward_fn(state, next_state) for m independent transitions: d_state, d_next_state [m][B][2]; d_reward [m],
 * d_termination [m] (1 = terminated or goal reached).  m = 0 is a no-op. */
int  rv_plan_reward(rv_world* w, const rv_plan_params* h_params, const float* d_state, const float* d_next_state,
                    int64_t m, float* d_reward /* [m] */, uint8_t* d_termination /* [m] */);
/* s candidate plans of h steps for each of the N envs.  d_plans [N][s][h][B][2] are the states AFTER each step;
 * d_state0 [N][B][2] is the state before the first one, NULL = the xy of the env's last observation.  Per plan, in
 * float32: ret = 0, disc = 1, len = h; for t in 0..h-1: (r, term) = reward_fn(s_t, s_t+1); ret += disc * r; if term:
 * len = t + 1, stop; disc *= gamma.  d_returns [N][s], d_lengths [N][s]; d_best [N]: the index of the largest return
 * of the env, the lowest index among equals.  Any of the three may be NULL. */
int  rv_plan_score(rv_world* w, const rv_plan_params* h_params, const float* d_state0, const float* d_plans,
                   int32_t s, int32_t h, float* d_returns /* [N][s] */, int32_t* d_lengths /* [N][s] */, int32_t* d_best /* [N] */);

/* ---- env states as data: save, restore, branch, and look-ahead with the simulator itself (no counterpart in the
 *      reference, whose planners get their candidate states from a learned dynamics model).  One env is one block of
 *      rv_state_bytes() bytes that holds no pointer and no env id: the bodies, the arm, its targets, the contact
 *      manifolds, the counters, the last observation and reward, the pending action and -- for an env that
 *      rv_step_poll left in the middle of an env.step() -- the step's progress.  Copying the block is copying the env;
 *      a restored env continues bit for bit as the saved one would have (every random draw is keyed by seed, global env
 *      id and the counters in the block; an env.step() with given actions draws nothing).  NOT in a block, hence neither
 *      saved nor branched: rv_set_auto_reset, the stream, the statistics of the last launch, the task-queue buffers.
 *      Blocks are only meaningful to the build that wrote them (rv_source_hash) and to worlds with the same rv_config
 *      apart from n_envs and env_id_offset.  Point clouds are sampled with the global env id of the env that is
 *      observed, so those of a branch differ from its source's; poses, rewards and depth renders do not.
 *      STREAM ORDERING: every call is asynchronous on the stream of the world that is WRITTEN (rv_state_save: the
 *      world that is read, into the caller's buffer).  rv_branch / rv_plan_simulate with two worlds on different
 *      streams: the copy waits, through an event, for everything the source's stream was given before the call, and
 *      the source's stream waits for the copy before it runs anything given to it after the call -- the source may be
 *      stepped right away.  Buffers the caller passes are ordered by the caller, as everywhere in this header. ---- */
int64_t rv_state_bytes(const rv_world* w);   /* bytes of one env block of the loaded build */
/* the N blocks of the world to d_buf (N x rv_state_bytes bytes, 4-byte aligned) */
int  rv_state_save(rv_world* w, void* d_buf);
/* env j takes block d_index[j] of the n_blocks blocks in d_buf; d_index == NULL: block j, and n_blocks must be N.  Index
 * -1 leaves env j as it is, and so does any other index outside [0, n_blocks): nothing outside the buffer is read. */
int  rv_state_load(rv_world* w, const void* d_buf, int32_t n_blocks, const int32_t* d_index /* [N] or NULL */);
/* env j of dst becomes a copy of env j / s of src: dst needs s x the envs of src.  RV_ERR_VALUE (and nothing changes)
 * unless the two rv_configs are equal apart from n_envs and env_id_offset and the worlds were made from the same
 * rv_scene on the same device.  The two may launch different builds of the env kernel (rv_env_kernel_build). */
int  rv_branch(rv_world* dst, rv_world* src, int32_t s);
/* s candidate action sequences of h steps for each of the N envs of src, tried out on the plan world (N x s envs):
 * rv_branch(plan, src, s), then h times { the actions of step t (as rv_set_actions); rv_step_macro; record }.  src is
 * only read.  d_actions [N][s][h][G][4]; d_states [N][s][h][RV_MAXB][2] (8-byte aligned) the xy of every body's
 * observed position after each step, zeros for absent bodies -- the d_plans of rv_plan_score, for any n_bodies;
 * d_rewards / d_dones [N][s][h] as rv_reward reports them after each step.  A branch whose episode ended earlier is
 * not stepped again: its later rows repeat its last state with reward 0, done 1.  Any output may be NULL.  PushEnv
 * worlds only; the conditions of rv_branch; h >= 1. */
int  rv_plan_simulate(rv_world* plan, rv_world* src, const float* d_actions, int32_t s, int32_t h,
                      float* d_states, float* d_rewards, uint8_t* d_dones);

/* ---- the two halves of a cross-entropy-method planner over rv_plan_simulate / rv_plan_score (no counterpart in the
 *      reference): per env a normal distribution over plans of h steps, d_mean / d_std [N][D], D = h * G * 4 floats.
 *      rv_cem_sample draws s candidates from it; rv_cem_refit fits it to the n_elites candidates with the largest
 *      returns.  The arithmetic (logarithm, Box-Muller, ranking order, moments) is written out operation for operation
 *      in csrc/rv_dev_cem.h.  A draw is Philox keyed by the world's seed, the GLOBAL env id, plan_index, iteration, the
 *      params' seed, the candidate and the float's index -- not by N, s, h or by what else is in the world: shards,
 *      partial batches and restored snapshots draw the same candidates.  Neither call reads more of an env than its
 *      global id, and neither changes any env state.  Asynchronous on the world's stream.  RV_ERR_VALUE, with nothing
 *      launched: s outside [1, RV_CEM_MAX_SAMPLES], h < 1, D > RV_CEM_MAX_DIM, plan_index outside [0, 2^24), iteration
 *      outside [0, 2^15) (the key packing), a missing required pointer, a buffer that is not 4-byte aligned, a grasp
 *      world; rv_cem_refit also: n_elites outside [1, s], alpha outside [0, 1), a negative or NaN min_std. ---- */
#define RV_CEM_MAX_SAMPLES 1024
#define RV_CEM_MAX_DIM 512
typedef struct rv_cem_params {
  int32_t plan_index, iteration;   /* Philox: the env.step() being planned, the CEM iteration */
  uint32_t seed;                   /* the policy's seed, on top of the world's                */
  int32_t keep_mean;               /* candidate 0 = the clamped mean                          */
  int32_t n_elites;                /* E, rv_cem_refit only                                    */
  float   alpha, min_std;          /* smoothing in [0,1), floor >= 0; rv_cem_refit only       */
} rv_cem_params;
/* d_actions [N][s][h][G][4] (the d_actions of rv_plan_simulate): fclamp(mean + std * z, -1, 1) with z standard normal,
 * |z| <= 5.77; with keep_mean, candidate 0 is fclamp(mean, -1, 1). */
int  rv_cem_sample(rv_world* w, const rv_cem_params* h_params, const float* d_mean, const float* d_std,
                   int32_t s, int32_t h, float* d_actions);
/* d_returns [N][s] ranks the candidates d_actions [N][s][h][G][4]: descending, the lower index first among equals, +-0
 * equal, NaNs after every number and by index.  Over the first E = n_elites, per float d and in rank order: m = the
 * mean, sd = the root of the mean squared deviation from m (ddof 0); then mean = alpha * mean + (1 - alpha) * m, std =
 * max(alpha * std + (1 - alpha) * sd, min_std), in place.  d_elite [N][E]: the elites' indices by rank, or NULL. */
int  rv_cem_refit(rv_world* w, const rv_cem_params* h_params, const float* d_actions, const float* d_returns,
                  int32_t s, int32_t h, float* d_mean, float* d_std, int32_t* d_elite /* [N][E] or NULL */);

/* ---- the depth sensor noise model of the reference's perception/depth_utils.py (gamma_noise, gaussian_noise) on
 *      [N][height][width] float buffers, N = the world's n_envs; both env kinds.  Per env: one multiplicative
 *      Gamma(k, 1/k) sample g, k = gamma_shape (Marsaglia-Tsang); with probability prob a grid of N(0, sigma^2) values,
 *      [height / R][width / R], upsampled x R by Pillow's bicubic resize and added where depth * g > 0.  The arithmetic is
 *      written out operation for operation in csrc/rv_dev_depth_noise.h.  A draw is Philox keyed by the world's seed, the
 *      GLOBAL env id, draw_index, the params' seed and the grid index -- not by N or by what else is in the world.  The
 *      call reads no more of an env than its global id and changes no env state.  d_depth_out may be d_depth_in.  The
 *      optional outputs record the draws: d_gamma [N], d_applied [N] (0 / 1), d_grid [N][height / R][width / R] (written
 *      for envs with applied != 0 and sigma > 0 only; NULL: the world keeps a scratch grid of its own).  Asynchronous on
 *      the world's stream.  RV_ERR_VALUE, with nothing launched: a missing required pointer, a buffer that is not 4-byte
 *      aligned, height or width < 1, rescale_factor outside [1, 8] or not dividing height and width, draw_index outside
 *      [0, 2^24), gamma_shape negative, NaN or in (0, 1), prob outside [0, 1] or NaN, sigma negative or NaN, more pixels
 *      than one launch takes. ---- */
typedef struct rv_depth_noise_params {
  int32_t  height, width;      /* of the depth buffers                         */
  int32_t  draw_index;         /* [0, 2^24): which observation of the env      */
  uint32_t seed;               /* the caller's stream                          */
  float    gamma_shape;        /* 0 = off, else >= 1                           */
  float    prob;               /* [0, 1]                                       */
  int32_t  rescale_factor;     /* R in [1, 8], divides height and width        */
  float    sigma;              /* >= 0, 0 = off                                */
} rv_depth_noise_params;
int  rv_depth_noise(rv_world* w, const rv_depth_noise_params* h_params, const float* d_depth_in,
                    float* d_depth_out /* may be d_depth_in */, float* d_gamma /* [N] or NULL */,
                    uint8_t* d_applied /* [N] or NULL */, float* d_grid /* [N][H/R][W/R] or NULL */);

/* ---- point clouds as the real sensor's branch of the reference segments them (camera_obs.py:90-124, 182-211): a plane
 *      fit that removes the table, DBSCAN on what is left, the C largest clusters sampled to P points each.  The three
 *      stages, their arithmetic and the Philox words are written out in csrc/rv_dev_segment.h.  Both
 *      calls work on a CHUNK of the world's envs, env_first .. env_first + env_count - 1, so that the caller bounds the
 *      [env_count][M][3] scratch; the draws are keyed by the global env id, not by the chunk.  Neither reads more of an
 *      env than its camera and its global id, neither changes env state; asynchronous on the world's stream.
 *      rv_deproject: every pixel of d_depth ([env_count][cam_height][cam_width], eye z) through Camera.deproject_pixel
 *      with the env's own calibration (rv_get_camera) into d_points [env_count][H * W][3]; d_valid [env_count][H * W] = 1
 *      where depth > 0 and the point is inside the config's crop (always, without a crop).
 *      rv_segment_cloud: d_points [env_count][M][3], d_valid [env_count][M] or NULL (all valid; a point with a non-finite
 *      coordinate is invalid either way).  Outputs: d_labels [env_count][M] (RV_SEG_INVALID, RV_SEG_PLANE, RV_SEG_SKIPPED,
 *      -1 = noise, >= 0 = cluster number), d_clouds [env_count][C][P][3], d_slot_labels / d_slot_counts [env_count][C] (the
 *      cluster number, -1 for an empty slot, and its member count), d_plane [env_count][4] (the unnormalised normal and the
 *      offset: n . p + d = 0 on the plane), d_info [env_count][RV_SEG_INFO_WORDS].  At most RV_SEG_MAXPTS survivors of the
 *      plane stage are clustered (more: that many evenly spaced, the rest RV_SEG_SKIPPED, RV_SEG_FLAG_OVERFLOW; min_samples
 *      is not rescaled).  RV_ERR_VALUE, with nothing launched: a NULL params or required buffer, a buffer that is not
 *      4-byte aligned, an env range outside the world, M outside [1, 2^24], num_hypotheses outside [0,
 *      RV_SEG_MAX_HYPOTHESES], num_clusters outside [1, RV_SEG_MAXSLOTS], num_points outside [1, 65536], eps or
 *      plane_thresh non-positive or non-finite, min_samples < 1, draw_index outside [0, 2^32). ---- */
#define RV_SEG_MAXPTS 8192
#define RV_SEG_MAX_HYPOTHESES 1024
#define RV_SEG_MAXSLOTS 16
#define RV_SEG_MAX_POINTS 65536
#define RV_SEG_INVALID (-3)
#define RV_SEG_PLANE   (-2)
#define RV_SEG_SKIPPED (-4)
#define RV_SEG_INFO_WORDS 8
#define RV_SEG_INFO_VALID 0      /* valid points                                  */
#define RV_SEG_INFO_PLANE 1      /* of them on the plane                          */
#define RV_SEG_INFO_SURVIVORS 2  /* valid, not on the plane                       */
#define RV_SEG_INFO_KEPT 3       /* of them clustered (<= RV_SEG_MAXPTS)          */
#define RV_SEG_INFO_CLUSTERS 4   /* clusters DBSCAN found                         */
#define RV_SEG_INFO_NOISE 5      /* kept points labelled -1                       */
#define RV_SEG_INFO_BEST_H 6     /* the winning hypothesis, -1: none              */
#define RV_SEG_INFO_FLAGS 7
#define RV_SEG_FLAG_NO_PLANE 1   /* T = 0, fewer than 3 valid points or every hypothesis void */
#define RV_SEG_FLAG_OVERFLOW 2   /* more than RV_SEG_MAXPTS survivors             */
#define RV_SEG_FLAG_BOUND 4      /* a loop bound ran out (never seen; the labels are then not to be trusted) */
#define RV_SEG_FLAG_FEWER 8      /* fewer clusters than slots: bodies merged, hidden or too small */
typedef struct rv_segment_params {
  int32_t num_hypotheses;      /* T in [0, RV_SEG_MAX_HYPOTHESES]; 0: no plane stage */
  float   plane_thresh;        /* > 0: the half width of the plane's band (m)  */
  float   eps;                 /* > 0: DBSCAN's radius (m)                     */
  int32_t min_samples;         /* >= 1, the point itself counts                */
  int32_t num_clusters;        /* C in [1, RV_SEG_MAXSLOTS]                    */
  int32_t num_points;          /* P in [1, RV_SEG_MAX_POINTS]                  */
  int64_t draw_index;          /* [0, 2^32): which observation of the env      */
} rv_segment_params;
int  rv_deproject(rv_world* w, int32_t env_first, int32_t env_count, const float* d_depth, float* d_points, uint8_t* d_valid);
int  rv_segment_cloud(rv_world* w, const rv_segment_params* h_params, int32_t env_first, int32_t env_count,
                      const float* d_points, const uint8_t* d_valid /* or NULL */, int32_t m,
                      int32_t* d_labels, float* d_clouds, int32_t* d_slot_labels, int32_t* d_slot_counts,
                      float* d_plane, int32_t* d_info);

/* ---- exactly C groups of the points rv_segment_cloud clustered: the reference's second cluster() call (camera_obs.py:
 *      208-210), scikit-learn's Ward agglomeration on the symmetrised k-nearest-neighbour graph cut at C clusters, then the
 *      grouping of rv_segment_cloud on those groups.  The definition is written out operation for operation in
 *      csrc/rv_dev_ward.h; the clustering is float64.  A chunk of envs like its two neighbours; reads no
 *      env state but the global env id, changes none; asynchronous on the world's stream.
 *      Input: d_points [env_count][M][3] and d_labels [env_count][M] as rv_segment_cloud wrote them; the points with a
 *      label >= 0 and finite coordinates are agglomerated (at most RV_WARD_MAXPTS: more are thinned to that many evenly
 *      spaced, the rest RV_SEG_SKIPPED in d_groups, RV_WARD_FLAG_OVERFLOW).  Outputs: d_groups [env_count][M] (the group
 *      number, groups numbered by ascending smallest member index; a negative label is kept), d_clouds
 *      [env_count][C][P][3] and d_slot_counts [env_count][C] (slot s = group s; fewer input points than groups: every
 *      point its own group, the other slots empty, RV_WARD_FLAG_FEWER), d_info [env_count][RV_WARD_INFO_WORDS].  The draws
 *      use the counter words of rv_segment_cloud's grouping, which this call replaces: where the groups are the clusters,
 *      d_clouds is bit for bit rv_segment_cloud's.  d_workspace: rv_ward_workspace_bytes(env_count) bytes of device
 *      memory, 8-byte aligned, contents don't matter (0 for env_count < 1).
 *      RV_ERR_VALUE, with nothing launched: a NULL params, buffer or workspace, a workspace that is too small or not
 *      8-byte aligned, a buffer that is not 4-byte aligned, an env range outside the world, M outside [1, 2^24],
 *      num_neighbors outside [1, RV_WARD_MAX_NEIGHBORS], num_groups outside [1, RV_SEG_MAXSLOTS], num_points outside
 *      [1, RV_SEG_MAX_POINTS], draw_index outside [0, 2^32). ---- */
#define RV_WARD_MAXPTS        2048
#define RV_WARD_MAX_NEIGHBORS 128
#define RV_WARD_INFO_WORDS    8
#define RV_WARD_INFO_INPUT 0        /* points with a label >= 0 and finite coordinates */
#define RV_WARD_INFO_KEPT 1         /* of them agglomerated (<= RV_WARD_MAXPTS)        */
#define RV_WARD_INFO_COMPONENTS 2   /* of the neighbour graph before completion        */
#define RV_WARD_INFO_EDGES_ADDED 3  /* by the completion                               */
#define RV_WARD_INFO_MERGES 4       /* merge steps taken                               */
#define RV_WARD_INFO_GROUPS 5       /* groups left                                     */
#define RV_WARD_INFO_RESERVED 6     /* 0                                               */
#define RV_WARD_INFO_FLAGS 7
#define RV_WARD_FLAG_OVERFLOW 2   /* more than RV_WARD_MAXPTS input points */
#define RV_WARD_FLAG_BOUND    4   /* a step found no adjacent pair: never expected, result not to be trusted */
#define RV_WARD_FLAG_FEWER    8   /* fewer input points than groups */
typedef struct rv_ward_params {
  int32_t num_neighbors;   /* k in [1, RV_WARD_MAX_NEIGHBORS]; the reference uses 100 */
  int32_t num_groups;      /* C in [1, RV_SEG_MAXSLOTS] */
  int32_t num_points;      /* P in [1, RV_SEG_MAX_POINTS] */
  int64_t draw_index;      /* [0, 2^32) */
} rv_ward_params;
size_t rv_ward_workspace_bytes(int32_t env_count);
int  rv_ward_groups(rv_world* w, const rv_ward_params* h_params, int32_t env_first, int32_t env_count,
                    const float* d_points, const int32_t* d_labels, int32_t m, void* d_workspace, size_t workspace_bytes,
                    int32_t* d_groups, float* d_clouds, int32_t* d_slot_counts, int32_t* d_info);

/* ---- s aimed pushes per env as proposals for look-ahead: the reference's HeuristicPushSampler.sample(position,
 *      body_mask, num_episodes, num_steps, num_samples) (heuristic_push_sampler.py:52-123) and a planning form of it.
 *      A push starts at least start_margin from every body and has its start or its end within motion_margin of its
 *      target body; an attempt is five uniform draws, tested as rv_policy_heuristic tests it; the arithmetic is written
 *      out operation for operation in csrc/rv_dev_push_sampler.h.  Read of an env: the positions, the body count and
 *      the two counters of its last observation; nothing is changed.
 *      RV_HP_EPISODE: the target is body num_episodes % n_bodies and the direction lies within 45 degrees of
 *      42 * num_episodes, as in the reference; the s candidates share rv_policy_heuristic's one sequence of attempts
 *      per env, candidate k starting behind the attempt candidate k - 1 stopped at, each with a budget of max_attempts:
 *      the first attempt that passes is taken (RV_HP_FOUND), else the last of the budget as drawn (RV_HP_EXHAUSTED).
 *      Candidate 0 is rv_policy_heuristic's push bit for bit.  plan_index, step and seed must be 0 and copies 1.
 *      RV_HP_SPREAD: env m of the world is copy m % copies of the SOURCE env with global id (env_id_offset + m) / copies
 *      (a world rv_branch filled with s copies per env has copies = s and s x the source's env_id_offset); candidate k
 *      has the index kg = (m % copies) * s + k, aims at body kg % n_bodies in a direction drawn from all of them, and has
 *      its own attempts and budget, Philox keyed by the world's seed, the source's global id, plan_index, step, the
 *      params' seed, kg and the attempt -- not by N, s, copies or by what else is in the world.  So s candidates of a
 *      world and one candidate of each of its s branches are the same bits while the observations are.
 *      RV_ERR_VALUE, with nothing launched: a grasp world, s outside [1, RV_HP_MAX_SAMPLES], copies < 1 or copies * s >
 *      RV_HP_MAX_SAMPLES, env_id_offset not a multiple of copies, max_attempts outside [1, RV_HP_MAX_ATTEMPTS], plan_index
 *      outside [0, 2^24), step outside [0, 64), an unknown mode, RV_HP_EPISODE with plan_index, step or seed not 0 or
 *      copies not 1, a negative or NaN margin, a missing required pointer, a buffer that is not 4-byte aligned. ---- */
#define RV_HP_MAX_SAMPLES 1024
#define RV_HP_MAX_ATTEMPTS 32768
#define RV_HP_EPISODE 0
#define RV_HP_SPREAD  1
#define RV_HP_FOUND 1
#define RV_HP_EXHAUSTED 0
typedef struct rv_push_proposal_params {
  int32_t  mode;                          /* RV_HP_EPISODE / RV_HP_SPREAD                               */
  int32_t  plan_index, step;              /* Philox: the env.step() being planned, the step of the plan */
  int32_t  copies;                        /* envs of this world per source env                          */
  int32_t  max_attempts;                  /* per candidate                                              */
  uint32_t seed;                          /* the policy's seed, on top of the world's                   */
  float    start_margin, motion_margin;   /* the reference's defaults: 0.05, 0.01                       */
} rv_push_proposal_params;
/* d_actions [M][s][G][4] (M = the world's n_envs): a candidate's (start x, start y, motion x, motion y) in each of the G
 * goal steps; d_status [M][s]: RV_HP_FOUND / RV_HP_EXHAUSTED.  Asynchronous on the world's stream. */
int  rv_policy_heuristic_multi(rv_world* w, const rv_push_proposal_params* h_params, int32_t s,
                               float* d_actions /* [M][s][G][4] */, int32_t* d_status /* [M][s] or NULL */);
/* rv_plan_simulate with the actions drawn instead of given, each step from the branch's own simulated state:
 * rv_branch(plan, src, s), then for t = 0 .. h - 1 { RV_HP_SPREAD proposals on the plan world, one per branch, with
 * copies = h_params->copies * s and step = h_params->step + t, into slice t of d_actions; the actions of step t;
 * rv_step_macro; record }.  Outputs, stream ordering and refusals as rv_plan_simulate, and those above for h_params (mode
 * must be RV_HP_SPREAD, step + h <= 64); the plan world needs env_id_offset = s x the source's.  src is only read. */
int  rv_plan_propose(rv_world* plan, rv_world* src, const rv_push_proposal_params* h_params, int32_t s, int32_t h,
                     float* d_actions /* out [N][s][h][G][4] */, float* d_states, float* d_rewards,
                     uint8_t* d_dones, int32_t* d_status /* [N][s][h] or NULL */);

/* ---- s route-following pushes per env as proposals for look-ahead (no counterpart in the reference): pushes that move
 *      body 0 -- the target of the crossing and insertion tasks -- one cell along the layout towards the goal.  The tiles
 *      span a grid of 8 x 8 cells, cell r * 8 + c centred at tile_offset + (r, c) * tile_size; walkable are the region
 *      and goal tiles (RV_TASK_CROSSING) or every cell but the region tiles, goal tiles included (RV_TASK_INSERTION).
 *      The route field D[64] (rv_get_route_field; a function of the rv_config alone, computed at a world's first use and
 *      kept) is the number of 4-neighbour hops through walkable cells to the nearest goal cell: 0 on a goal cell, 255 on
 *      a cell that is not walkable or reaches no goal.  A push aims from body 0 at the centre of the neighbour, one hop
 *      closer to the goal, of the walkable cell nearest to body 0 (at that cell's own centre on a goal cell, at the nearest
 *      goal centre where no goal is reached), rotated by a jitter angle; it starts `back` behind the body on that line,
 *      `lat` to its side, and is (distance to the aim + back) * f long.  An attempt draws the jitter from +- angle_jitter,
 *      back from [back_lo, back_hi], lat from +- lateral and f from [length_lo, length_hi] -- four uniforms of one Philox
 *      block keyed as RV_HP_SPREAD keys its attempts, on a stream id of its own -- and passes if its start is farther than
 *      start_margin from every movable body; the first that passes is taken (RV_HP_FOUND), else the last of max_attempts
 *      as drawn (RV_HP_EXHAUSTED).  With keep_nominal the candidate with index kg = 0 draws nothing: no jitter, back =
 *      (back_lo + back_hi) / 2, lat = 0, f = 1.  copies, kg and the source env's global id are those of RV_HP_SPREAD, so
 *      s candidates of a world and one candidate of each of its s branches are the same bits while the observations are.
 *      An env whose body 0 is not movable gets a zero action and RV_HP_EXHAUSTED.  Read of an env: the positions and the
 *      body count of its last observation; nothing is changed.  The arithmetic is written out operation for operation in
 *      csrc/rv_dev_push_route.h.  The first of these calls on a world launches the field's kernel and waits for it, once
 *      (not inside a stream capture); after that they are asynchronous on the world's stream.
 *      RV_ERR_VALUE, with nothing launched: a grasp world, a task other than crossing or insertion, n_goal == 0 (or a
 *      tile count outside [0, RV_MAXTILES]), a region or goal tile that is no integer pair of the 8 x 8 grid, s outside
 *      [1, RV_HP_MAX_SAMPLES], copies < 1 or copies * s > RV_HP_MAX_SAMPLES, env_id_offset not a multiple of copies,
 *      max_attempts outside [1, RV_HP_MAX_ATTEMPTS], plan_index outside [0, 2^24), step outside [0, 64), a negative or NaN
 *      start_margin, angle_jitter or lateral, back_lo > back_hi, length_lo > length_hi, length_lo < 0 (a NaN among them
 *      too), a missing required pointer, a buffer that is not 4-byte aligned. ---- */
typedef struct rv_push_route_params {
  int32_t  plan_index, step;              /* Philox: the env.step() being planned, the step of the plan */
  int32_t  copies;                        /* envs of this world per source env                          */
  int32_t  max_attempts;                  /* per candidate                                              */
  uint32_t seed;                          /* the policy's seed, on top of the world's                   */
  int32_t  keep_nominal;                  /* candidate kg = 0 is the push without jitter                */
  float    start_margin;                  /* the start's clearance from every body                      */
  float    angle_jitter;                  /* radians, to either side of the aim direction               */
  float    back_lo, back_hi;              /* how far behind body 0 the push starts                      */
  float    lateral;                       /* the start's offset to either side of the aim line          */
  float    length_lo, length_hi;          /* the push length as a fraction of (distance + back)         */
} rv_push_route_params;
int  rv_get_route_field(rv_world* w, uint8_t* d_out /* [64] */);
/* d_actions [M][s][G][4], d_status [M][s] as rv_policy_heuristic_multi.  Asynchronous on the world's stream. */
int  rv_policy_route_multi(rv_world* w, const rv_push_route_params* h_params, int32_t s,
                           float* d_actions /* [M][s][G][4] */, int32_t* d_status /* [M][s] or NULL */);
/* rv_plan_propose with route-following pushes: the same loop, step t drawn with copies = h_params->copies * s and step =
 * h_params->step + t from the branch's own simulated state.  Outputs, stream ordering and refusals as rv_plan_propose,
 * and those above for h_params (step + h <= 64). */
int  rv_plan_propose_route(rv_world* plan, rv_world* src, const rv_push_route_params* h_params, int32_t s, int32_t h,
                           float* d_actions /* out [N][s][h][G][4] */, float* d_states, float* d_rewards,
                           uint8_t* d_dones, int32_t* d_status /* [N][s][h] or NULL */);

/* ---- Simulator.step x n (simulator.py:94-103): ControllableBody.update +
 *      BulletPhysics.step (bullet_physics.py:106-109), no phase machine. ---- */
int  rv_step_sub(rv_world* w, int32_t n_substeps);
/* ---- Simulator.wait_until_stable (simulator.py:325-376) over all movables. */
int  rv_wait_until_stable(rv_world* w, float lin_thresh, float ang_thresh,
                          int32_t check_after, int32_t min_stable, int32_t max_steps);

/* ---- state getters: Body.pose/linear_velocity/angular_velocity
 *      (body.py:72-125, bullet_physics.py:197-249); Joint.position/velocity
 *      (bullet_physics.py:635-663); Link.pose (bullet_physics.py:460-473). ---- */
int  rv_get_body_state(rv_world* w, float* d_out /* [N][RV_MAXB][13] */);
int  rv_set_body_state(rv_world* w, const float* d_in /* [N][RV_MAXB][13] */);
int  rv_get_body_params(rv_world* w, float* d_out /* [N][RV_MAXB][8]: active,shape,scale,mass,friction,frozen,0,0 */);
int  rv_set_body_params(rv_world* w, const float* d_in);
int  rv_get_joint_state(rv_world* w, float* d_out /* [N][RV_NJ][2] */);
int  rv_set_joint_state(rv_world* w, const float* d_in /* [N][RV_NJ][2] */);
int  rv_get_link_poses(rv_world* w, float* d_out /* [N][RV_NFRAME][7] */);
#define RV_NCOUNTERS 10
int  rv_get_env_counters(rv_world* w, int32_t* d_out /* [N][RV_NCOUNTERS]: sim_steps, num_steps, num_episodes, phase, done, is_safe, is_effective, substeps_last, awake_substeps_last, narrowphase_pairs_last */);

/* ---- ControllableBody.set_target_joint_positions / set_target_link_pose
 *      (controllable_body.py:263-345) via RobotCommand (simulator.py:226-244). */
/*      timeout (s) / threshold (rad): <= 0 selects the robot config's LIMB_TIMEOUT /
 *      LIMB_POSITION_THRESHOLD (sawyer_sim.py:201-204). */
int  rv_set_joint_targets(rv_world* w, const float* d_q /* [N][RV_NLIMB] */, float timeout, float threshold);
int  rv_set_link_target(rv_world* w, const float* d_pose /* [N][7] pos+xyzw */, float timeout, float threshold);
/* ---- SawyerSim.move_along_gripper_path (sawyer_sim.py:310-360) -> ControllableBody.set_target_link_poses
 *      (controllable_body.py:322-345): 1 <= n_poses <= RV_MAXQ gripper poses per env, followed one after the other
 *      (the next pose is taken when the IK solution of the current one is reached). */
int  rv_set_link_path(rv_world* w, const float* d_poses /* [N][n_poses][7] pos+xyzw */, int32_t n_poses, float timeout, float threshold);
/* ---- SawyerSim.is_limb_ready / is_gripper_ready (sawyer_sim.py:394-408; ControllableBody.is_ready,
 *      controllable_body.py:565-595): like the reference's query it retires link / joint targets that are done
 *      (reached, timed out, path exhausted).  The gripper is ready 0.5 s of simulated time after rv_grip. */
int  rv_get_robot_ready(rv_world* w, uint8_t* d_out /* [N][2]: limb ready, gripper ready */);
/* ControllableBody.set_max_joint_velocities (controllable_body.py:357-372), the robot command SawyerSim.move_to_joint_positions /
 * move_to_gripper_pose / move_along_gripper_path send with every motion (sawyer_sim.py:212-220, 285-293, 336-344: `speed` x
 * joint.max_velocity, default speed = LIMB_MAX_VELOCITY_RATIO): the speed limit (rad/s, > 0) of each of the seven limb joints
 * for the targets that are being followed.  rv_set_joint_targets / rv_set_link_target / rv_set_link_path put the configured
 * ratio back, so a per-call speed is set AFTER the target it belongs to (both before the next Simulator.step). */
int  rv_set_max_joint_velocities(rv_world* w, const float* d_vmax /* [N][RV_NLIMB] */);
/* ---- BulletPhysics.position_control_array (bullet_physics.py:1061-1104):
 *      POSITION_CONTROL motor targets (gains POSITION_GAIN / VELOCITY_GAIN,
 *      controllable_body.py:17-18) for the joints whose mask byte is non-zero
 *      (d_mask == NULL: all RV_NJ joints).  Bypasses the JointTarget layer. */
int  rv_set_motor_targets(rv_world* w, const float* d_q /* [N][RV_NJ] */, const uint8_t* d_mask /* [N][RV_NJ] or NULL */);
/* ---- SawyerSim.grip (sawyer_sim.py:362-392): value in [0, 1], 0 = open. */
int  rv_grip(rv_world* w, float value);
/* Simulator.add_constraint / Constraint.pose, max_force setters / remove_constraint
 * (simulator.py:166-224; bullet_physics.py:748-957 createConstraint / changeConstraint /
 * removeConstraint), for the constraint ControllableConstraint servoes
 * (controllable_constraint.py:21-170): a FIXED joint between the frame frame7 (host float[7]:
 * position + xyzw quaternion in the body frame; NULL = the body frame itself) of movable body
 * `body` and the world frame target7, applying at most max_force newtons per row.  Every env of
 * the world gets it; calling again moves the world frame (the servo does that every substep);
 * max_force < 0 removes the constraint.  (A movable child / a point-to-point joint: rv_set_constraint_ex.) */
int  rv_set_constraint(rv_world* w, int32_t body, const float* frame7, const float* target7, float max_force);
/* The same with the other arguments of BulletPhysics.add_constraint (bullet_physics.py:748-806: createConstraint(parent,
 * parentLink, child, childLink, jointType, jointAxis, parentFramePosition, childFramePosition, ...)): `child` = -1 (the
 * world) or another movable body slot -- child_frame7 is then given in the CHILD's frame and every row acts on both
 * bodies, which stay awake together; joint_type RV_JOINT_FIXED (six rows), RV_JOINT_POINT2POINT (pybullet
 * JOINT_POINT2POINT: the three linear rows, the bodies turn freely about the pivot) or RV_JOINT_PRISMATIC (the body
 * slides along the X AXIS of the frame it is tied to -- child_frame7's orientation: two linear rows across that axis
 * and the three angular rows; a jointAxis other than x is a rotation of both frames, which the HipPhysics mirror
 * applies) or RV_JOINT_REVOLUTE (the fourth type of the reference's JOINT_TYPES_MAPPING, bullet_physics.py:20-25: a hinge about
 * the X AXIS of the frame -- the three linear rows at the pivot and two angular rows across the axis).  Other pybullet joint
 * types (gear ...) are not in the reference's mapping: RV_ERR_NOTIMPL.  `child` = RV_CHILD_LINK(f): frame f of the ARM is the
 * other party (createConstraint with a (body, link) entity, bullet_physics.py:773-790: e.g. an object attached to the hand) --
 * child_frame7 is given in that link frame, which moves kinematically (the rows see the link's twist, the link takes no
 * impulse); fixed and point2point joints. */
#define RV_CHILD_LINK(f)     (RV_MAXB + (f))
#define RV_JOINT_REVOLUTE    0   /* pybullet.JOINT_REVOLUTE */
#define RV_JOINT_PRISMATIC   1   /* pybullet.JOINT_PRISMATIC */
#define RV_JOINT_FIXED       4   /* pybullet.JOINT_FIXED */
#define RV_JOINT_POINT2POINT 5   /* pybullet.JOINT_POINT2POINT */
int  rv_set_constraint_ex(rv_world* w, int32_t body, int32_t child, int32_t joint_type, const float* frame7,
                          const float* child_frame7, float max_force);
/* BulletPhysics.set_gravity (bullet_physics.py:129-137): the gravity vector of every env of
 * the world from now on (host float[3]) */
int  rv_set_gravity(rv_world* w, const float* gravity);
/* BulletPhysics.set_link_dynamics / set_body_dynamics, lateral friction only (bullet_physics.py:560-600,
 * 318-350; grasp_4dof_env.py:262-293 switches the finger-tip and table friction between the phases of a
 * grasp): the lateral friction of the two finger-tip pads and of the table top of every env of the world;
 * a negative value leaves that coefficient as it is */
int  rv_set_friction(rv_world* w, float mu_finger, float mu_table);
/* ---- ControllableBody.reset_targets (controllable_body.py:347-350): drop the
 *      link / joint targets; the motors keep their last commanded positions. */
int  rv_reset_targets(rv_world* w);
/* ---- BulletPhysics.compute_inverse_kinematics (bullet_physics.py:1203-1262). */
int  rv_compute_ik(rv_world* w, const float* d_pose /* [N][7] */, float* d_q /* [N][RV_NLIMB] */);

/* ---- Simulator.check_contact / BulletPhysics.get_contact_points
 *      (simulator.py:246-287, bullet_physics.py:1268-1304).
 *      d_out: uint8[N][2+RV_MAXB]: arm-table, arm-any-movable, arm-movable[b]. */
int  rv_query_contacts(rv_world* w, uint8_t* d_out);
/* ---- BulletPhysics.get_contact_points / pybullet.getContactPoints (bullet_physics.py:1262-1304), the records
 *      behind Simulator.check_contact and Body.contacts (simulator.py:246-287), batched: one record per contact
 *      point of every env, filtered by the query (-1 = any) and oriented so that body_a is body A.
 *      Body codes: a body slot 0..RV_MAXB-1, RV_CP_TABLE, RV_CP_ARM.  Links: -1, or for the arm the
 *      link frame of the collider (scenes.LINK_NAMES index); link_a / link_b only with the arm.
 *      d_ids   int32[N][capacity][4]          bodyA, bodyB, linkA, linkB
 *      d_data  float[N][capacity][RV_CP_NF]   positionOnA[3], positionOnB[3], contactNormalOnB[3], contactDistance,
 *                                             normalForce, lateralFriction1, lateralFrictionDir1[3],
 *                                             lateralFriction2, lateralFrictionDir2[3]  (forces: impulse / dt)
 *      d_count int32[N]                       number of matching records (may exceed capacity: only the first
 *                                             `capacity` are written, in manifold-slot / point order)
 *      Gated so that for every pair "count > 0" equals the rv_query_contacts / manifold-count hit test; while the
 *      arm-table flag is set a last record (arm, table, links -1, NaN positions and distance, normal +z, zero forces)
 *      stands for it.  RV_ERR_VALUE: capacity outside [1, RV_CP_MAX], an unknown body code, a link for a body
 *      that is not the arm.  Asynchronous on the world's stream. */
#define RV_CP_NF    19
#define RV_CP_TABLE RV_MAXB
#define RV_CP_ARM   (RV_MAXB + 1)
#define RV_CP_MAX   (RV_NMAN * 4 + 1)
typedef struct rv_contact_query {
  int32_t body_a, link_a, body_b, link_b;
} rv_contact_query;
int  rv_get_contact_points(rv_world* w, const rv_contact_query* q, int capacity,
                           int32_t* d_ids, float* d_data, int32_t* d_count);
/* ---- the camera calibration an env's observations are rendered with (Camera.intrinsics / translation / rotation,
 *      camera.py:150-168; the camera-calibration observations of camera_obs.py:241-320): rv_config's values plus the
 *      noise drawn at that env's last reset (cam_noise). */
int  rv_get_camera(rv_world* w, float* d_out /* [N][17]: fx, fy, cx, cy, skew, rotation[9] row-major, translation[3] */);
/* Number of manifold points per manifold slot, for parity tests. */
int  rv_get_manifold_counts(rv_world* w, int32_t* d_out /* [N][RV_NMAN] */);

/* ---- observations (push_env.py:169-236): PoseObs('position') pose_obs.py:53-73,
 *      attribute obs attribute_obs.py:16-115, SegmentedPointCloudObs
 *      camera_obs.py:182-238: ray-cast depth + segmentation, deprojection, P pixels per body
 *      emitted in the order of their Philox keys -- a random permutation, so the row order within
 *      a body's cloud carries no meaning; bodies with more than RV_PC_MAXPIX = 2048 visible pixels
 *      are sampled with a stride, or from RV_PC_MAXPIX evenly spaced ones where the stride leaves fewer than P).  NULL pointers are skipped. */
typedef struct rv_obs_buffers {
  float*   d_position;     /* [N][RV_MAXB][3]                                   */
  float*   d_body_mask;    /* [N][RV_MAXB]                                      */
  int64_t* d_num_episodes; /* [N]                                               */
  int64_t* d_num_steps;    /* [N]                                               */
  int64_t* d_layout_id;    /* [N]                                               */
  int64_t* d_is_safe;      /* [N]                                               */
  int64_t* d_is_effective; /* [N]                                               */
  float*   d_point_cloud;  /* [N][RV_MAXB][num_points][3]                       */
  /* the other PoseObs modalities (pose_obs.py:53-73), zero rows for absent bodies */
  float*   d_pose;         /* [N][RV_MAXB][6]  position + static-xyz Euler      */
  float*   d_pose2d;       /* [N][RV_MAXB][3]  x, y, yaw                        */
  float*   d_yaw_cossin;   /* [N][RV_MAXB][2]  cos(yaw), sin(yaw)               */
} rv_obs_buffers;
int  rv_observe(rv_world* w, const rv_obs_buffers* obs);

/* ---- the complete record of a rollout: what generate_episode writes per transition
 *      (episode_generation.py:47-67: state, ACTION, reward, info, where the state of an episode's
 *      first transition is the observation env.reset() returned).  Beyond rv_rollout_record: the
 *      action every env.step() executed, and for every step that an auto-reset preceded, the
 *      observation of the freshly reset state (rows of the other steps are zero).  With them the
 *      [n_steps][N] buffers split into the reference's episodes without losing a transition. */
typedef struct rv_rollout_extra {
  float*   d_actions;        /* [n_steps][N][G][4]  (G = max(num_goal_steps, 1)); NULL: skipped */
  uint8_t* d_reset;          /* [n_steps][N]  1 = the env was reset right before this step      */
  rv_obs_buffers reset_obs;  /* [n_steps][N]...  observation env.reset() returned; NULL members skipped */
} rv_rollout_extra;
int  rv_rollout_record_full(rv_world* w, int32_t n_steps, int32_t first_macro_index, int32_t auto_reset,
                            float* d_rewards, uint8_t* d_dones, const rv_obs_buffers* step_obs,
                            const rv_rollout_extra* extra);
/* Who rendered the point clouds of the last rv_rollout_record / rv_rollout_record_full of this world (for tests).  In the
 * plain launch of the one-wave-per-SIMD build, workgroups whose env has finished render the clouds of snapshot rows that
 * are stored already; the rows they leave are rendered after the kernel.  by_tail + by_residual = n_steps x N (0 and 0
 * when that call took no point clouds); by_tail = 0 on the other build, through the task queues, and with RV_PC_TAIL=0
 * in the environment (read per launch).  RV_PC_TAIL_CAP=n: a finished workgroup renders n rows at most.  The clouds
 * are the same bytes whoever renders them.  Synchronises the world's stream; h_ pointers are host memory. */
int  rv_last_tail_renders(rv_world* w, int32_t* h_by_tail, int32_t* h_by_residual);

/* ---- CameraObs 'depth' / 'segmask' (camera_obs.py:33-88; BulletCamera._frames,
 *      bullet_camera.py:188-235) of the simulated depth camera: eye-space depth (0 where
 *      nothing is hit) and segmentation (body index, RV_MAXB = table, RV_MAXB + 1 = the arm's link boxes, 255 = nothing).
 *      The arm is drawn as its ten link collider boxes and occludes bodies.  Either pointer may be NULL. */
int  rv_render(rv_world* w, float* d_depth /* [N][cam_height][cam_width] */, uint8_t* d_segmask /* same shape */);
/* CameraObs 'rgb' (camera_obs.py:33-88; bullet_camera.py:188-235): the same ray cast, flat colours
 * per body slot / table / background, Lambert-shaded with the normal of the face that is hit under
 * one fixed directional light (BUILD-CHOSEN colours: the reference draws random rgba per body,
 * push_env.py:436).  The arm's link boxes are drawn in a flat grey. */
int  rv_render_rgb(rv_world* w, uint8_t* d_rgb /* [N][cam_height][cam_width][3] */);
/* ---- Free camera views of chosen envs (no counterpart in the reference's observation path; its PushEnv draws a second,
 *      "recording" camera through pybullet, push_env.py:282-327, 1155-1162).  View v looks at env h_env_index[v] through
 *      camera row v of h_cameras -- the layout of rv_get_camera: fx, fy, cx, cy, skew, rotation[9] row-major,
 *      translation[3] -- at height x width pixels: V images of any size from any pose, of any subset of the envs (an env
 *      may be looked at by several views).  Pixel (u, v) of a view is what rv_render / rv_render_rgb compute for that env
 *      with the camera of its snapshot replaced by the row: views that repeat the envs' own cameras at the config's size
 *      reproduce those two bit for bit.  Depth 0, segmask 255 and the background colour where nothing is hit beyond
 *      cam_near.  Any output pointer may be NULL, not all three.
 *      supersample = s in 1..4 (rgb only): the host scales the row to the s-times larger image in float32 -- fx' = s fx,
 *      fy' = s fy, skew' = s skew, cx' = s cx + (s - 1) / 2, cy' = s cy + (s - 1) / 2 -- and output pixel (u, v) is the
 *      integer box filter (sum + s s / 2) / (s s), per channel, of the s x s pixels (s u + i, s v + j) of that image.
 *      h_params, h_env_index and h_cameras are HOST arrays: everything is checked before anything is launched
 *      (RV_ERR_VALUE, outputs untouched: a NULL among them, no output, n_views / height / width outside [1,
 *      RV_VIEW_MAX_VIEWS / RV_VIEW_MAX_SIDE], supersample outside [1, RV_VIEW_MAX_SUPERSAMPLE], an env index outside
 *      [0, N), a row with a non-finite entry or fx == 0 / fy == 0, d_depth not 4-byte aligned, depth or segmask with
 *      s > 1) and then copied to a buffer of the world on its stream; the arrays may be reused on return.  The call reads
 *      the envs only: it changes no env state and leaves a pending rv_step_begin / rv_step_poll step pending. */
#define RV_VIEW_MAX_VIEWS 4096
#define RV_VIEW_MAX_SIDE 4096
#define RV_VIEW_MAX_SUPERSAMPLE 4
typedef struct rv_view_params { int32_t n_views, height, width, supersample; } rv_view_params;
int  rv_render_view(rv_world* w, const rv_view_params* h_params,
                    const int32_t* h_env_index /* [V] */, const float* h_cameras /* [V][17] */,
                    uint8_t* d_rgb /* [V][height][width][3] or NULL */, float* d_depth /* [V][height][width] or NULL */,
                    uint8_t* d_segmask /* [V][height][width] or NULL */);

/* ---- PushReward.get_reward (push_reward.py:377-405, 272-374) of the last
 *      macro step, and RobotEnv done flag (robot_env.py:257-259). ---- */
int  rv_reward(rv_world* w, float* d_reward /* [N] */, uint8_t* d_done /* [N] */);
int  rv_get_episode_returns(rv_world* w, float* d_returns /* [N] */);

/* ---- stats of the last rv_step_macro / rv_reset launch (host struct). ---- */
int  rv_get_stats(rv_world* w, rv_macro_stats* h_stats);
/* HIP-event duration of the last rv_step_macro / rv_step_sub / rv_reset kernel
 * on the world's stream, in milliseconds (used by bench.py's roofline). */
int  rv_last_kernel_ms(rv_world* w, float* h_ms);

/* ---- zero-copy, READ-ONLY views of the resident state (the
 *      scalar getters of body.py:72-125 / joint.py:41-92 batched).  The env
 *      blocks are env-major: field f of env i lives at
 *      d_envs + i * env_stride_bytes + off_f.  Valid until rv_destroy; contents
 *      change with every stepping call on the world's stream. ---- */
typedef struct rv_state_view {
  const void* d_envs;
  int64_t env_stride_bytes;
  int64_t off_body;        /* float[RV_MAXB][13]  pos3 quat4(xyzw) lin3 ang3     */
  int64_t off_active;      /* int32[RV_MAXB]                                     */
  int64_t off_joint_q;     /* float[RV_NJ]                                       */
  int64_t off_joint_qd;    /* float[RV_NJ]                                       */
  int64_t off_link_pos;    /* float[RV_NFRAME][3]                                */
  int64_t off_link_quat;   /* float[RV_NFRAME][4]                                */
  int64_t off_obs_pos;     /* float[RV_MAXB][3]   PoseObs('position') snapshot   */
  int64_t off_table_z;     /* float                                              */
} rv_state_view;
int  rv_get_state_ptrs(rv_world* w, rv_state_view* h_out);

/* sha256 (hex) of the sources the loaded binary was compiled from, baked in at
 * build time (robovat_amd/lib.py: source_hash()); __graft_entry__.smoke()
 * compares it with the hash of the sources that travelled with the binary. */
const char* rv_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* ROVAT_H_ */
