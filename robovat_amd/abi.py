"""ctypes mirror of ``include/rovat.h`` (struct layouts and capacities).

Both the product library (``librovat_hip.so``) and the test oracle take these
structures by pointer, so one Python object configures either side.
"""
import ctypes as C

RV_MAXB = 4
RV_MAXH = 4
RV_MAXV = 16
RV_MAXP = 28
RV_PC_MAXPIX = 2048
RV_MAX_SHAPES = 16
RV_NJ = 9
RV_NLIMB = 7
RV_NFRAME = 10
RV_NCOL = 10
RV_MAXTILES = 24
RV_MAXG = 4
RV_MAXQ = 8
RV_AP_MAX_RADIUS = 32
RV_AP_MAX_EDGES = 4096
RV_AP_MAX_SAMPLES = 64
RV_AP_OK, RV_AP_NO_EDGES, RV_AP_NO_PAIRS, RV_AP_ALL_REJECTED, RV_AP_TOO_MANY_EDGES = 1, 0, -1, -2, -3


def RV_CHILD_LINK(f):
    """child argument of rv_set_constraint_ex for frame f of the arm (include/rovat.h)"""
    return RV_MAXB + int(f)

RV_NBB = RV_MAXB * (RV_MAXB - 1) // 2
RV_NMAN = 2 * RV_MAXB + RV_NBB
RV_BODY_STRIDE = 13
# rv_get_contact_points (include/rovat.h): record width, body codes of the table and the arm, records per env
RV_CP_NF = 19
RV_CP_TABLE = RV_MAXB
RV_CP_ARM = RV_MAXB + 1
RV_CP_MAX = RV_NMAN * 4 + 1
RV_NCOUNTERS = 10
# rv_env_kernel_build: the build of the env kernel a world launches (k_env / k_env_occ2)
RV_ENV_BUILD_OCC1, RV_ENV_BUILD_OCC2 = 1, 2

RV_OK, RV_ERR_VALUE, RV_ERR_STATE, RV_ERR_HIP, RV_ERR_NOTIMPL = 0, 1, 2, 3, 4
RV_TASK_NONE, RV_TASK_CLEARING, RV_TASK_INSERTION, RV_TASK_CROSSING = 0, 1, 2, 3
TASK_IDS = {None: 0, 'data_collection': 0, 'clearing': 1, 'insertion': 2,
            'crossing': 3}
PHASES = ['initial', 'pre', 'start', 'motion', 'post', 'offstage', 'done']
GRASP_PHASES = ['initial', 'overhead', 'prestart', 'start', 'end', 'postend', 'done']
RV_ENV_PUSH, RV_ENV_GRASP = 0, 1

f32, i32, u32, i64 = C.c_float, C.c_int32, C.c_uint32, C.c_int64


class rv_shape(C.Structure):
    _fields_ = [
        ('n_hulls', i32),
        ('n_verts', i32 * RV_MAXH),
        ('verts', ((f32 * 3) * RV_MAXV) * RV_MAXH),
        ('inertia_k', f32 * 3),
        ('radius', f32),
        ('n_planes', i32 * RV_MAXH),
        ('planes', ((f32 * 4) * RV_MAXP) * RV_MAXH),
    ]


class rv_arm(C.Structure):
    _fields_ = [
        ('base_pos', f32 * 3),
        ('base_quat', f32 * 4),
        ('jpos', (f32 * 3) * (RV_NLIMB + 1)),
        ('jquat', (f32 * 4) * (RV_NLIMB + 1)),
        ('q_lo', f32 * RV_NJ), ('q_hi', f32 * RV_NJ),
        ('v_max', f32 * RV_NJ),
        ('a_max', f32 * RV_NJ),
        ('finger_y0', f32 * 2),
        ('col_frame', i32 * RV_NCOL),
        ('col_center', (f32 * 3) * RV_NCOL),
        ('col_half', (f32 * 3) * RV_NCOL),
        ('inv_tau_max', f32 * RV_NJ),
        ('link_mass', f32 * (RV_NLIMB + 1)), ('link_com', (f32 * 3) * (RV_NLIMB + 1)), ('link_inertia', (f32 * 3) * (RV_NLIMB + 1)),
    ]


class rv_scene(C.Structure):
    _fields_ = [
        ('n_shapes', i32),
        ('shapes', rv_shape * RV_MAX_SHAPES),
        ('arm', rv_arm),
    ]


class rv_config(C.Structure):
    _fields_ = [
        ('n_envs', i32), ('env_id_offset', i32),
        ('seed_lo', u32), ('seed_hi', u32),
        ('dt', f32), ('gravity_z', f32),
        ('solver_iters', i32),
        ('erp', f32), ('slop', f32), ('margin', f32), ('breaking', f32),
        ('warmstart', f32), ('max_pushout', f32),
        ('lin_damp', f32), ('ang_damp', f32),
        ('contact_query_dist', f32),
        ('solver_tol', f32), ('sleep_lin', f32), ('sleep_ang', f32), ('sleep_steps', i32),
        ('sleep_pos_win', f32), ('sleep_rot_win', f32),
        ('np_gate', f32), ('np_max_age', i32),
        ('table_center', f32 * 2), ('table_half', f32 * 2),
        ('table_thickness', f32), ('table_z', f32),
        ('table_height_range', f32 * 2),
        ('table_friction', f32), ('arm_friction', f32), ('fall_depth', f32),
        ('n_bodies_min', i32), ('n_bodies_max', i32),
        ('scale_range', f32 * 2), ('mass_range', f32 * 2),
        ('friction_range', f32 * 2),
        ('margin_xy', f32),
        ('pose_lo', f32 * 6), ('pose_hi', f32 * 6),
        ('drop_mass', f32), ('drop_friction', f32), ('safe_drop_height', f32),
        ('n_movable_shapes', i32), ('movable_shapes', i32 * RV_MAX_SHAPES),
        ('n_target_shapes', i32), ('target_shapes', i32 * RV_MAX_SHAPES),
        ('task', i32), ('layout_id', i32), ('use_tiles', i32),
        ('tile_size', f32), ('tile_offset', f32 * 2),
        ('n_region', i32), ('n_goal', i32), ('n_target', i32),
        ('n_obstacle', i32),
        ('region', (f32 * 2) * RV_MAXTILES),
        ('goal', (f32 * 2) * RV_MAXTILES),
        ('target', (f32 * 2) * RV_MAXTILES),
        ('obstacle', (f32 * 2) * RV_MAXTILES),
        ('kp', f32), ('kd', f32), ('velocity_threshold', f32),
        ('limb_max_velocity_ratio', f32), ('limb_timeout', f32),
        ('limb_position_threshold', f32),
        ('ik_iters', i32),
        ('ik_damping', f32), ('ik_residual', f32), ('ik_max_step', f32),
        ('neutral_positions', f32 * RV_NLIMB),
        ('offstage_positions', f32 * RV_NLIMB),
        ('open_gripper_when_reset', i32),
        ('cspace_low', f32 * 3), ('cspace_high', f32 * 3),
        ('translation_x', f32), ('translation_y', f32),
        ('finger_tip_offset', f32), ('gripper_safe_height', f32),
        ('min_delta_position', f32), ('min_delta_angle', f32),
        ('workspace_x_range', f32), ('workspace_y_range', f32),
        ('steps_check', i32), ('max_phase_steps', i32),
        ('max_motion_steps', i32), ('max_offstage_steps', i32),
        ('num_goal_steps', i32), ('max_steps', i32),
        ('success_thresh', f32),
        ('num_points', i32),
        ('cam_height', i32), ('cam_width', i32),
        ('cam_intrinsics', f32 * 5),
        ('cam_rotation', f32 * 9),
        ('cam_translation', f32 * 3),
        ('cam_near', f32),
        ('use_crop', i32),
        ('crop_min', f32 * 3), ('crop_max', f32 * 3),
        ('env_type', i32), ('finger_dynamics', i32),
        ('finger_mass', f32), ('finger_max_force', f32),
        ('grasp_cuboid_low', f32 * 3), ('grasp_cuboid_high', f32 * 3),
        ('overhead_positions', f32 * RV_NLIMB),
        ('max_action_steps', i32), ('end_effector_step', f32),
        ('grasp_mu_descend', f32 * 2), ('grasp_mu_lift', f32 * 2),
        ('ground_z', f32), ('ground_friction', f32), ('rolling_friction', f32), ('wake_gap', f32), ('deact_lin', f32), ('deact_ang', f32), ('deact_steps', i32),
        ('gravity_xy', f32 * 2), ('arm_effort_limit', i32), ('limb_dynamics', i32), ('solver_stall', i32), ('solver_tol_rest', f32),
        ('cam_noise', f32 * 17),
        ('wall_use', i32), ('wall_shape', i32), ('wall_scale', f32), ('wall_pose', f32 * 7),
    ]


class rv_macro_stats(C.Structure):
    _fields_ = [
        ('substeps', i64), ('env_steps', i64), ('unsafe', i64),
        ('ineffective', i64), ('useful', i64), ('successes', i64),
        ('episodes_done', i64), ('max_substeps', i64), ('awake_substeps', i64),
    ]


class rv_obs_buffers(C.Structure):
    _fields_ = [
        ('d_position', C.c_void_p), ('d_body_mask', C.c_void_p),
        ('d_num_episodes', C.c_void_p), ('d_num_steps', C.c_void_p),
        ('d_layout_id', C.c_void_p), ('d_is_safe', C.c_void_p),
        ('d_is_effective', C.c_void_p), ('d_point_cloud', C.c_void_p),
        ('d_pose', C.c_void_p), ('d_pose2d', C.c_void_p), ('d_yaw_cossin', C.c_void_p),
    ]


class rv_rollout_extra(C.Structure):
    _fields_ = [('d_actions', C.c_void_p), ('d_reset', C.c_void_p), ('reset_obs', rv_obs_buffers)]


class rv_state_view(C.Structure):
    _fields_ = [
        ('d_envs', C.c_void_p), ('env_stride_bytes', i64),
        ('off_body', i64), ('off_active', i64), ('off_joint_q', i64), ('off_joint_qd', i64),
        ('off_link_pos', i64), ('off_link_quat', i64), ('off_obs_pos', i64), ('off_table_z', i64),
    ]


class rv_antipodal_params(C.Structure):
    _fields_ = [
        ('friction_coef', f32), ('depth_grad_thresh', f32), ('depth_grad_gaussian_sigma', f32),
        ('downsample_rate', i32), ('max_rejection_samples', i32), ('use_crop', i32), ('crop', i32 * 4),
        ('min_dist_from_boundary', f32), ('min_grasp_dist', f32), ('angle_dist_weight', f32),
        ('depth_samples_per_grasp', i32), ('min_depth_offset', f32), ('max_depth_offset', f32),
        ('depth_sample_window_height', f32), ('depth_sample_window_width', f32),
        ('gripper_width', f32), ('cone_cos', f32), ('gauss_radius', i32),
        ('gauss_weights', f32 * (RV_AP_MAX_RADIUS + 1)),
    ]


class rv_contact_query(C.Structure):
    _fields_ = [('body_a', i32), ('link_a', i32), ('body_b', i32), ('link_b', i32)]


class rv_plan_params(C.Structure):
    _fields_ = [
        ('n_bodies', i32), ('is_high_level', i32), ('use_dense_reward', i32), ('use_time_penalty', i32),
        ('goal_reward', f32), ('termination_reward', f32), ('dense_reward', f32), ('time_reward', f32),
        ('gamma', f32),
    ]


RV_CEM_MAX_SAMPLES = 1024
RV_CEM_MAX_DIM = 512


class rv_cem_params(C.Structure):
    _fields_ = [
        ('plan_index', i32), ('iteration', i32), ('seed', C.c_uint32), ('keep_mean', i32), ('n_elites', i32),
        ('alpha', f32), ('min_std', f32),
    ]


# rv_cem_sample: world, h_params, d_mean, d_std, s, h, d_actions; rv_cem_refit: world, h_params, d_actions, d_returns, s, h,
# d_mean, d_std, d_elite (include/rovat.h); lib.load() binds them from here
CEM_API = {
    'rv_cem_sample': (C.c_int, [C.c_void_p, C.POINTER(rv_cem_params), C.c_void_p, C.c_void_p, i32, i32, C.c_void_p]),
    'rv_cem_refit': (C.c_int, [C.c_void_p, C.POINTER(rv_cem_params), C.c_void_p, C.c_void_p, i32, i32,
                               C.c_void_p, C.c_void_p, C.c_void_p]),
}


RV_DN_MAX_DRAW_INDEX = 1 << 24
RV_DN_MAX_RESCALE = 8


class rv_depth_noise_params(C.Structure):
    _fields_ = [
        ('height', i32), ('width', i32), ('draw_index', i32), ('seed', C.c_uint32), ('gamma_shape', f32), ('prob', f32),
        ('rescale_factor', i32), ('sigma', f32),
    ]


# rv_depth_noise: world, h_params, d_depth_in, d_depth_out, d_gamma, d_applied, d_grid (include/rovat.h); lib.load() binds
# it from here
DEPTH_NOISE_API = {
    'rv_depth_noise': (C.c_int, [C.c_void_p, C.POINTER(rv_depth_noise_params), C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
}


RV_SEG_MAXPTS = 8192
RV_SEG_MAX_HYPOTHESES = 1024
RV_SEG_MAXSLOTS = 16
RV_SEG_MAX_POINTS = 65536
RV_SEG_INVALID, RV_SEG_PLANE, RV_SEG_SKIPPED = -3, -2, -4
RV_SEG_INFO_WORDS = 8
(RV_SEG_INFO_VALID, RV_SEG_INFO_PLANE, RV_SEG_INFO_SURVIVORS, RV_SEG_INFO_KEPT, RV_SEG_INFO_CLUSTERS, RV_SEG_INFO_NOISE,
 RV_SEG_INFO_BEST_H, RV_SEG_INFO_FLAGS) = range(8)
RV_SEG_FLAG_NO_PLANE, RV_SEG_FLAG_OVERFLOW, RV_SEG_FLAG_BOUND, RV_SEG_FLAG_FEWER = 1, 2, 4, 8


class rv_segment_params(C.Structure):
    _fields_ = [
        ('num_hypotheses', i32), ('plane_thresh', f32), ('eps', f32), ('min_samples', i32), ('num_clusters', i32),
        ('num_points', i32), ('draw_index', C.c_int64),
    ]


# rv_deproject: world, env_first, env_count, d_depth, d_points, d_valid; rv_segment_cloud: world, h_params, env_first,
# env_count, d_points, d_valid, m, d_labels, d_clouds, d_slot_labels, d_slot_counts, d_plane, d_info (include/rovat.h);
# lib.load() binds them from here
SEGMENT_API = {
    'rv_deproject': (C.c_int, [C.c_void_p, i32, i32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'rv_segment_cloud': (C.c_int, [C.c_void_p, C.POINTER(rv_segment_params), i32, i32, C.c_void_p, C.c_void_p, i32,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


RV_WARD_MAXPTS = 2048
RV_WARD_MAX_NEIGHBORS = 128
RV_WARD_INFO_WORDS = 8
(RV_WARD_INFO_INPUT, RV_WARD_INFO_KEPT, RV_WARD_INFO_COMPONENTS, RV_WARD_INFO_EDGES_ADDED, RV_WARD_INFO_MERGES,
 RV_WARD_INFO_GROUPS, RV_WARD_INFO_RESERVED, RV_WARD_INFO_FLAGS) = range(8)
RV_WARD_FLAG_OVERFLOW, RV_WARD_FLAG_BOUND, RV_WARD_FLAG_FEWER = 2, 4, 8


class rv_ward_params(C.Structure):
    _fields_ = [
        ('num_neighbors', i32), ('num_groups', i32), ('num_points', i32), ('draw_index', C.c_int64),
    ]


# rv_ward_workspace_bytes: env_count; rv_ward_groups: world, h_params, env_first, env_count, d_points, d_labels, m,
# d_workspace, workspace_bytes, d_groups, d_clouds, d_slot_counts, d_info (include/rovat.h); lib.load() binds them from here
WARD_API = {
    'rv_ward_workspace_bytes': (C.c_size_t, [i32]),
    'rv_ward_groups': (C.c_int, [C.c_void_p, C.POINTER(rv_ward_params), i32, i32, C.c_void_p, C.c_void_p, i32, C.c_void_p,
                                 C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


RV_HP_MAX_SAMPLES = 1024
RV_HP_MAX_ATTEMPTS = 32768
RV_HP_EPISODE, RV_HP_SPREAD = 0, 1
RV_HP_FOUND, RV_HP_EXHAUSTED = 1, 0


class rv_push_proposal_params(C.Structure):
    _fields_ = [
        ('mode', i32), ('plan_index', i32), ('step', i32), ('copies', i32), ('max_attempts', i32), ('seed', C.c_uint32),
        ('start_margin', f32), ('motion_margin', f32),
    ]


# rv_policy_heuristic_multi: world, h_params, s, d_actions, d_status; rv_plan_propose: plan world, source world, h_params,
# s, h, d_actions, d_states, d_rewards, d_dones, d_status (include/rovat.h); lib.load() binds them from here
PUSH_PROPOSAL_API = {
    'rv_policy_heuristic_multi': (C.c_int, [C.c_void_p, C.POINTER(rv_push_proposal_params), i32, C.c_void_p, C.c_void_p]),
    'rv_plan_propose': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(rv_push_proposal_params), i32, i32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


RV_PR_GRID = 8
RV_PR_NONE = 255


class rv_push_route_params(C.Structure):
    _fields_ = [
        ('plan_index', i32), ('step', i32), ('copies', i32), ('max_attempts', i32), ('seed', C.c_uint32), ('keep_nominal', i32),
        ('start_margin', f32), ('angle_jitter', f32), ('back_lo', f32), ('back_hi', f32), ('lateral', f32),
        ('length_lo', f32), ('length_hi', f32),
    ]


# rv_get_route_field: world, d_out; rv_policy_route_multi: world, h_params, s, d_actions, d_status; rv_plan_propose_route:
# plan world, source world, h_params, s, h, d_actions, d_states, d_rewards, d_dones, d_status (include/rovat.h); lib.load()
# binds them from here
PUSH_ROUTE_API = {
    'rv_get_route_field': (C.c_int, [C.c_void_p, C.c_void_p]),
    'rv_policy_route_multi': (C.c_int, [C.c_void_p, C.POINTER(rv_push_route_params), i32, C.c_void_p, C.c_void_p]),
    'rv_plan_propose_route': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(rv_push_route_params), i32, i32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


# the env-state entry points of include/rovat.h (rv_state_*/ rv_branch / rv_plan_simulate): name -> (restype, argtypes);
# lib.load() binds them from here.  Worlds and device buffers are void pointers.
STATE_API = {
    'rv_state_bytes': (i64, [C.c_void_p]),
    'rv_state_save': (C.c_int, [C.c_void_p, C.c_void_p]),
    'rv_state_load': (C.c_int, [C.c_void_p, C.c_void_p, i32, C.c_void_p]),
    'rv_branch': (C.c_int, [C.c_void_p, C.c_void_p, i32]),
    'rv_plan_simulate': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, i32, i32, C.c_void_p, C.c_void_p, C.c_void_p]),
}


# rv_policy_antipodal_multi (include/rovat.h): world, d_depth, h_params, macro_index, num_samples, d_image_grasps,
# d_actions4, d_count, d_status; lib.load() binds it from here
ANTIPODAL_API = {
    'rv_policy_antipodal_multi': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(rv_antipodal_params), i32, i32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


RV_GC_MAX_SIDE = 256
RV_GC_MAX_STEP = 16


class rv_grasp_crop_params(C.Structure):
    _fields_ = [
        ('height', i32), ('width', i32), ('crop_height', i32), ('crop_width', i32), ('step', i32), ('reserved', i32 * 3),
    ]


# rv_grasp_crops (include/rovat.h): world, h_params, d_depth, d_grasps, k, d_images, d_grasp_depths; lib.load() binds it
# from here
GRASP_CROP_API = {
    'rv_grasp_crops': (C.c_int, [C.c_void_p, C.POINTER(rv_grasp_crop_params), C.c_void_p, C.c_void_p, i32,
                                 C.c_void_p, C.c_void_p]),
}


RV_GQ_MIN_SIDE = 8
RV_GQ_MAX_SIDE = 32
RV_GQ_MAX_CHANNELS = 16
RV_GQ_MAX_FEATURES = 128
RV_GQ_MAX_POSE = 32


class rv_grasp_quality_model(C.Structure):
    _fields_ = [
        ('height', i32), ('width', i32), ('c1', i32), ('c2', i32), ('f1', i32), ('f2', i32), ('p', i32), ('reserved', i32),
        ('im_mean', C.c_float), ('im_inv_std', C.c_float), ('z_mean', C.c_float), ('z_inv_std', C.c_float),
    ]


# rv_grasp_quality_weight_count: h_model; rv_grasp_quality: world, h_model, d_weights, d_images, d_grasp_depths, k,
# d_logits (include/rovat.h); lib.load() binds them from here
GRASP_QUALITY_API = {
    'rv_grasp_quality_weight_count': (C.c_int64, [C.POINTER(rv_grasp_quality_model)]),
    'rv_grasp_quality': (C.c_int, [C.c_void_p, C.POINTER(rv_grasp_quality_model), C.c_void_p, C.c_void_p, C.c_void_p, i32,
                                   C.c_void_p]),
}


RV_GQ_MAX_BATCH = 4096


class rv_adam_params(C.Structure):
    _fields_ = [
        ('lr', C.c_float), ('beta1', C.c_float), ('beta2', C.c_float), ('eps', C.c_float), ('corr1', C.c_float),
        ('corr2', C.c_float), ('reserved', i32 * 2),
    ]


# the training step of the grasp-quality network (include/rovat.h); lib.load() binds them from here
GRASP_TRAIN_API = {
    'rv_grasp_quality_train_workspace_floats': (C.c_int64, [C.POINTER(rv_grasp_quality_model), C.c_int64]),
    'rv_grasp_quality_forward_train': (C.c_int, [C.c_void_p, C.POINTER(rv_grasp_quality_model), C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    'rv_grasp_quality_backward': (C.c_int, [C.c_void_p, C.POINTER(rv_grasp_quality_model), C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    'rv_adam_step': (C.c_int, [C.c_void_p, C.POINTER(rv_adam_params), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
}


RV_GR_MAX_ITERATION = 1 << 26
RV_GR_MAX_MACRO_INDEX = 1 << 24


class rv_grasp_refine_params(C.Structure):
    _fields_ = [
        ('height', i32), ('width', i32), ('macro_index', i32), ('iteration', i32), ('seed', C.c_uint32), ('n_elites', i32),
        ('sigma_center', C.c_float), ('sigma_angle', C.c_float), ('sigma_depth', C.c_float), ('reserved', i32 * 3),
    ]


# rv_grasp_refine (include/rovat.h): world, h_params, h_sampler, d_depth, d_grasps, d_scores, d_count, d_status, k,
# d_grasps_out, d_actions4_out, d_parent, d_count_out; lib.load() binds it from here
GRASP_REFINE_API = {
    'rv_grasp_refine': (C.c_int, [C.c_void_p, C.POINTER(rv_grasp_refine_params), C.POINTER(rv_antipodal_params),
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, i32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


RV_VIEW_MAX_VIEWS = 4096
RV_VIEW_MAX_SIDE = 4096
RV_VIEW_MAX_SUPERSAMPLE = 4


class rv_view_params(C.Structure):
    _fields_ = [('n_views', i32), ('height', i32), ('width', i32), ('supersample', i32)]


# rv_render_view (include/rovat.h): world, h_params, h_env_index, h_cameras, d_rgb, d_depth, d_segmask; lib.load() binds it
# from here
VIEW_API = {
    'rv_render_view': (C.c_int, [C.c_void_p, C.POINTER(rv_view_params), C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
}

# rv_last_tail_renders (include/rovat.h): world, h_by_tail, h_by_residual -- who rendered the point clouds of the last
# recorded rollout (the rollout kernel's finished workgroups / the launch after it); lib.load() binds it from here
PC_TAIL_API = {
    'rv_last_tail_renders': (C.c_int, [C.c_void_p, C.POINTER(i32), C.POINTER(i32)]),
}


def bind_state_api(handle):
    """restype / argtypes of the STATE_API functions on a loaded librovat_hip.so"""
    for name, (res, args) in STATE_API.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = res, list(args)


def config_key(cfg):
    """The bytes of an rv_config that two worlds must share to exchange env blocks: everything but n_envs and
    env_id_offset (rv_branch compares the same)."""
    c = rv_config.from_buffer_copy(bytes(cfg))
    c.n_envs = 0
    c.env_id_offset = 0
    return bytes(c)


def assign(arr, values):
    """Copy a (nested) python/numpy sequence into a ctypes array."""
    for i, v in enumerate(values):
        if hasattr(v, '__len__'):
            assign(arr[i], v)
        else:
            arr[i] = v
