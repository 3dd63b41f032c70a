"""Loader and thin Python binding of ``librovat_hip.so`` (``include/rovat.h``).

The library is the product: there is NO CPU fallback.  Importing this module
is cheap; ``load()`` raises ``RuntimeError`` if the shared object has not been
built (``python -c "import __graft_entry__ as g; g.build()"``) and
``World(...)`` raises if no HIP device is present.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from robovat_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('RV_LIB', os.path.join(_HERE, 'librovat_hip.so'))
CSRC = os.path.join(_HERE, 'csrc')
HIPCC_FLAGS = ['-O3', '-std=c++17', '--offload-arch=gfx950', '-ffp-contract=off',
               '-fPIC', '-shared']

# every symbol include/rovat.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    'rv_create', 'rv_destroy', 'rv_last_error', 'rv_set_stream', 'rv_synchronize',
    'rv_num_envs', 'rv_reset', 'rv_set_actions', 'rv_step_macro', 'rv_policy_random',
    'rv_policy_heuristic', 'rv_rollout', 'rv_rollout_async', 'rv_step_sub', 'rv_wait_until_stable', 'rv_get_body_state',
    'rv_set_body_state', 'rv_get_body_params', 'rv_set_body_params',
    'rv_get_joint_state', 'rv_set_joint_state', 'rv_get_link_poses',
    'rv_get_env_counters', 'rv_set_joint_targets', 'rv_set_link_target',
    'rv_compute_ik', 'rv_query_contacts', 'rv_get_manifold_counts', 'rv_observe',
    'rv_reward', 'rv_get_episode_returns', 'rv_get_stats', 'rv_last_kernel_ms',
    'rv_reset_targets', 'rv_get_state_ptrs', 'rv_source_hash', 'rv_set_motor_targets', 'rv_grip',
    'rv_rollout_record', 'rv_render', 'rv_set_gravity', 'rv_rollout_record_full', 'rv_step_begin', 'rv_step_poll', 'rv_set_constraint', 'rv_render_rgb', 'rv_set_friction', 'rv_set_auto_reset',
    'rv_set_constraint_ex', 'rv_set_link_path', 'rv_get_robot_ready', 'rv_get_camera', 'rv_set_max_joint_velocities',
    'rv_policy_antipodal', 'rv_policy_antipodal_multi', 'rv_get_contact_points', 'rv_env_kernel_build',
    'rv_plan_reward', 'rv_plan_score',
    'rv_state_bytes', 'rv_state_save', 'rv_state_load', 'rv_branch', 'rv_plan_simulate',
    'rv_cem_sample', 'rv_cem_refit',
    'rv_depth_noise',
    'rv_policy_heuristic_multi', 'rv_plan_propose',
    'rv_get_route_field', 'rv_policy_route_multi', 'rv_plan_propose_route',
    'rv_grasp_crops',
    'rv_grasp_quality_weight_count', 'rv_grasp_quality',
    'rv_grasp_quality_train_workspace_floats', 'rv_grasp_quality_forward_train', 'rv_grasp_quality_backward', 'rv_adam_step',
    'rv_grasp_refine',
    'rv_render_view',
    'rv_deproject', 'rv_segment_cloud',
    'rv_ward_workspace_bytes', 'rv_ward_groups',
    'rv_last_tail_renders',
]

_EXC = {abi.RV_ERR_VALUE: ValueError, abi.RV_ERR_STATE: RuntimeError,
        abi.RV_ERR_HIP: RuntimeError, abi.RV_ERR_NOTIMPL: NotImplementedError}
_lib = None


SOURCES = [os.path.join(CSRC, n) for n in sorted(os.listdir(CSRC)) if n.endswith(('.hip', '.h'))]
SOURCES.append(os.path.join(_HERE, '..', 'include', 'rovat.h'))


def source_hash():
    """sha256 over the sources librovat_hip.so is compiled from (file names and bytes)."""
    import hashlib
    h = hashlib.sha256()
    for path in SOURCES:
        h.update(os.path.basename(path).encode())
        with open(path, 'rb') as f:
            h.update(f.read())
    return h.hexdigest()


def built_source_hash():
    """The hash baked into the loaded binary (rv_source_hash)."""
    lib = load()
    return lib.rv_source_hash().decode()


def build(force=False, verbose=False):
    """Compile csrc/rv_kernels.hip for gfx950 into librovat_hip.so (in-tree).
    The sha256 of the sources is baked into the binary (rv_source_hash)."""
    if (not force and os.path.exists(LIB_PATH) and
            all(os.path.getmtime(d) <= os.path.getmtime(LIB_PATH) for d in SOURCES)):
        return LIB_PATH
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    compile_lib(LIB_PATH, hipcc=hipcc, verbose=verbose)
    return LIB_PATH


def compile_lib(out, extra=(), hipcc='/opt/rocm/bin/hipcc', verbose=False):
    """The two translation units (rv_kernels.hip: C ABI + the register-rich env kernel; rv_kernels_occ2.hip: the
    env kernel for two waves per SIMD) compiled side by side, then linked into one shared object.  Objects and the
    linked library are made in a private temporary directory next to `out` and the library is moved into place with
    one rename: concurrent builds (the multi-rank tests) never see each other's half-written files, and a failed
    translation unit leaves neither a running compiler nor objects behind."""
    import shutil
    import tempfile
    srcs = [os.path.join(CSRC, 'rv_kernels.hip'), os.path.join(CSRC, 'rv_kernels_occ2.hip')]
    flags = [f for f in HIPCC_FLAGS if f != '-shared'] + ['-DRV_SOURCE_HASH="%s"' % source_hash()] + list(extra)
    tmp = tempfile.mkdtemp(prefix='.build_', dir=os.path.dirname(os.path.abspath(out)))
    procs = []
    try:
        objs = []
        for src in srcs:
            obj = os.path.join(tmp, os.path.basename(src) + '.o')
            cmd = [hipcc] + flags + ['-c', src, '-o', obj]
            if verbose:
                print(' '.join(cmd))
            procs.append(subprocess.Popen(cmd)); objs.append(obj)
        codes = [p.wait() for p in procs]          # (every compiler is waited for before an error is raised)
        if any(codes):
            raise subprocess.CalledProcessError(next(c for c in codes if c), 'hipcc')
        linked = os.path.join(tmp, os.path.basename(out))
        cmd = [hipcc, '--offload-arch=gfx950', '-fPIC', '-shared'] + objs + ['-o', linked]
        if verbose:
            print(' '.join(cmd))
        subprocess.run(cmd, check=True)
        os.replace(linked, out)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill(); p.wait()
        shutil.rmtree(tmp, ignore_errors=True)


def load():
    """dlopen librovat_hip.so; fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            'librovat_hip.so is not built (%s). Run __graft_entry__.build(); '
            'there is no CPU fallback.' % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.rv_last_error.restype = C.c_char_p
    lib.rv_source_hash.restype = C.c_char_p
    lib.rv_create.argtypes = [C.POINTER(abi.rv_config), C.POINTER(abi.rv_scene),
                              C.c_int, C.POINTER(C.c_void_p)]
    for name in SYMBOLS:
        fn = getattr(lib, name)
        if name not in ('rv_last_error', 'rv_source_hash'):
            fn.restype = C.c_int
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    lib.rv_destroy.argtypes = [vp]
    lib.rv_set_stream.argtypes = [vp, vp]
    lib.rv_synchronize.argtypes = [vp]
    lib.rv_num_envs.argtypes = [vp]
    lib.rv_env_kernel_build.argtypes = [vp]
    lib.rv_reset.argtypes = [vp, vp]
    lib.rv_step_macro.argtypes = [vp]
    lib.rv_step_sub.argtypes = [vp, i32]
    lib.rv_step_begin.argtypes = [vp, vp, vp]
    lib.rv_step_poll.argtypes = [vp, i32, i32, vp, C.POINTER(abi.rv_obs_buffers), vp, vp]
    lib.rv_rollout.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.rv_rollout_async.argtypes = [vp, i32, i32, vp]
    lib.rv_rollout_record.argtypes = [vp, i32, i32, i32, vp, vp, C.POINTER(abi.rv_obs_buffers)]
    lib.rv_rollout_record_full.argtypes = [vp, i32, i32, i32, vp, vp, C.POINTER(abi.rv_obs_buffers), C.POINTER(abi.rv_rollout_extra)]
    lib.rv_wait_until_stable.argtypes = [vp, f32, f32, i32, i32, i32]
    lib.rv_policy_random.argtypes = [vp, i32, vp]
    lib.rv_policy_heuristic.argtypes = [vp, i32, vp]
    lib.rv_observe.argtypes = [vp, C.POINTER(abi.rv_obs_buffers)]
    lib.rv_reward.argtypes = [vp, vp, vp]
    lib.rv_compute_ik.argtypes = [vp, vp, vp]
    lib.rv_get_stats.argtypes = [vp, C.POINTER(abi.rv_macro_stats)]
    lib.rv_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.rv_reset_targets.argtypes = [vp]
    lib.rv_render.argtypes = [vp, vp, vp]
    lib.rv_render_rgb.argtypes = [vp, vp]
    lib.rv_set_motor_targets.argtypes = [vp, vp, vp]
    lib.rv_grip.argtypes = [vp, f32]
    lib.rv_set_gravity.argtypes = [vp, C.POINTER(C.c_float)]
    lib.rv_set_friction.argtypes = [vp, f32, f32]
    lib.rv_set_auto_reset.argtypes = [vp, i32]
    lib.rv_set_constraint.argtypes = [vp, i32, C.POINTER(C.c_float), C.POINTER(C.c_float), f32]
    lib.rv_set_constraint_ex.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float), f32]
    lib.rv_get_state_ptrs.argtypes = [vp, C.POINTER(abi.rv_state_view)]
    lib.rv_set_joint_targets.argtypes = [vp, vp, f32, f32]
    lib.rv_set_link_target.argtypes = [vp, vp, f32, f32]
    lib.rv_set_link_path.argtypes = [vp, vp, i32, f32, f32]
    lib.rv_get_robot_ready.argtypes = [vp, vp]
    lib.rv_set_max_joint_velocities.argtypes = [vp, vp]
    lib.rv_get_camera.argtypes = [vp, vp]
    lib.rv_policy_antipodal.argtypes = [vp, vp, C.POINTER(abi.rv_antipodal_params), i32, vp, vp, vp]
    lib.rv_get_contact_points.argtypes = [vp, C.POINTER(abi.rv_contact_query), i32, vp, vp, vp]
    lib.rv_plan_reward.argtypes = [vp, C.POINTER(abi.rv_plan_params), vp, vp, C.c_int64, vp, vp]
    lib.rv_plan_score.argtypes = [vp, C.POINTER(abi.rv_plan_params), vp, vp, i32, i32, vp, vp, vp]
    for name in ('rv_set_actions', 'rv_get_body_state', 'rv_set_body_state',
                 'rv_get_body_params', 'rv_set_body_params', 'rv_get_joint_state',
                 'rv_set_joint_state', 'rv_get_link_poses', 'rv_get_env_counters',
                 'rv_query_contacts', 'rv_get_manifold_counts', 'rv_get_episode_returns'):
        getattr(lib, name).argtypes = [vp, vp]
    abi.bind_state_api(lib)
    for api in (abi.ANTIPODAL_API, abi.CEM_API, abi.DEPTH_NOISE_API, abi.PUSH_PROPOSAL_API, abi.PUSH_ROUTE_API,
                abi.GRASP_CROP_API, abi.GRASP_QUALITY_API, abi.GRASP_TRAIN_API, abi.GRASP_REFINE_API, abi.VIEW_API,
                abi.SEGMENT_API, abi.WARD_API, abi.PC_TAIL_API):
        for name, (res, args) in api.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, list(args)
    _lib = lib
    return lib


def antipodal_params(config=None):
    """The ``rv_antipodal_params`` of an AntipodalGrasp4DofPolicy config (``configs.ANTIPODAL_GRASP_4DOF_POLICY_CONFIG``
    layout: SAMPLER keys + GRIPPER_WIDTH).  The Gaussian weights and the friction cone's cosine are computed here in
    float64 and rounded to float32; the library checks the values (ValueError)."""
    import math
    from robovat_amd import configs
    cfg = configs.AttrDict(config or configs.ANTIPODAL_GRASP_4DOF_POLICY_CONFIG)
    s = cfg['SAMPLER']
    p = abi.rv_antipodal_params()
    p.friction_coef = float(s['FRICTION_COEF'])
    p.depth_grad_thresh = float(s['DEPTH_GRAD_THRESH'])
    p.depth_grad_gaussian_sigma = sigma = float(s['DEPTH_GRAD_GAUSSIAN_SIGMA'])
    p.downsample_rate = int(s['DOWNSAMPLE_RATE']) if float(s['DOWNSAMPLE_RATE']) == int(s['DOWNSAMPLE_RATE']) else -1
    p.max_rejection_samples = int(s['MAX_REJECTION_SAMPLES'])
    p.use_crop = int(s.get('CROP') is not None)
    if p.use_crop:
        abi.assign(p.crop, [int(v) for v in s['CROP']])
    p.min_dist_from_boundary = float(s['MIN_DIST_FROM_BOUNDARY'])
    p.min_grasp_dist = float(s.get('MIN_GRASP_DIST', 0.0))
    p.angle_dist_weight = float(s.get('ANGLE_DIST_WEIGHT', 0.0))
    p.depth_samples_per_grasp = int(s['DEPTH_SAMPLES_PER_GRASP'])
    p.min_depth_offset = float(s['MIN_DEPTH_OFFSET'])
    p.max_depth_offset = float(s['MAX_DEPTH_OFFSET'])
    p.depth_sample_window_height = float(s['DEPTH_SAMPLE_WINDOW_HEIGHT'])
    p.depth_sample_window_width = float(s['DEPTH_SAMPLE_WINDOW_WIDTH'])
    p.gripper_width = float(cfg.get('GRIPPER_WIDTH', 0.0) or 0.0)
    p.cone_cos = math.cos(math.atan(p.friction_coef))
    # scipy.ndimage.gaussian_filter1d: radius int(4 sigma + 0.5), normalised exp(-x^2 / 2 sigma^2); sigma ~ 0: identity
    if sigma <= 1e-15:
        p.gauss_radius = 0
        p.gauss_weights[0] = 1.0
    else:
        radius = int(4.0 * sigma + 0.5)
        p.gauss_radius = radius
        if radius <= abi.RV_AP_MAX_RADIUS:
            x = np.arange(-radius, radius + 1)
            phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
            phi /= phi.sum()
            abi.assign(p.gauss_weights, phi[radius:].astype(np.float32).tolist())
    return p


def _override(p, who, overrides):
    """``p`` with the fields named in ``overrides`` set, each value converted to the field's type; a name that is no field
    of the struct, or its ``reserved`` words, is a TypeError"""
    names = [n for n, _ in p._fields_ if n != 'reserved']
    for k, v in overrides.items():
        if k not in names:
            raise TypeError('%s: unknown field %r' % (who, k))
        setattr(p, k, type(getattr(p, k))(v))
    return p


def plan_params(**overrides):
    """The ``rv_plan_params`` of ``get_reward_fn(..., is_planning=True)`` with the reference's defaults
    (push_reward.py:272-281): n_bodies 4, low level, goal 100, termination -100, dense 1, time -1, both terms on;
    gamma 1 (``rv_plan_score`` sums the rewards).  Keyword arguments override fields."""
    p = abi.rv_plan_params(n_bodies=abi.RV_MAXB, is_high_level=0, use_dense_reward=1, use_time_penalty=1,
                           goal_reward=100.0, termination_reward=-100.0, dense_reward=1.0, time_reward=-1.0, gamma=1.0)
    return _override(p, 'plan_params', overrides)


def cem_params(**overrides):
    """An ``rv_cem_params``: plan_index 0, iteration 0, seed 0, keep_mean on, one elite, alpha 0 (no smoothing),
    min_std 0.  Keyword arguments override fields."""
    p = abi.rv_cem_params(plan_index=0, iteration=0, seed=0, keep_mean=1, n_elites=1, alpha=0.0, min_std=0.0)
    return _override(p, 'cem_params', overrides)


def push_proposal_params(mode='spread', **overrides):
    """An ``rv_push_proposal_params``: ``mode`` 'spread' / 'episode' (or RV_HP_SPREAD / RV_HP_EPISODE), plan_index 0, step
    0, copies 1, max_attempts 20000, seed 0 and the reference's margins (start 0.05, motion 0.01).  Keyword arguments
    override fields."""
    modes = {'episode': abi.RV_HP_EPISODE, 'spread': abi.RV_HP_SPREAD}
    p = abi.rv_push_proposal_params(mode=modes.get(mode, mode), plan_index=0, step=0, copies=1, max_attempts=20000, seed=0,
                                    start_margin=0.05, motion_margin=0.01)
    return _override(p, 'push_proposal_params', overrides)


def push_route_params(**overrides):
    """An ``rv_push_route_params``: plan_index 0, step 0, copies 1, max_attempts 256, seed 0, keep_nominal 1, start_margin
    0.05, angle_jitter 0.3, back_lo 0.08, back_hi 0.16, lateral 0.02, length_lo 0.8, length_hi 1.2 (the spreads are
    unmeasured defaults around the one push that was tried).  Keyword arguments override fields."""
    p = abi.rv_push_route_params(plan_index=0, step=0, copies=1, max_attempts=256, seed=0, keep_nominal=1, start_margin=0.05,
                                 angle_jitter=0.3, back_lo=0.08, back_hi=0.16, lateral=0.02, length_lo=0.8, length_hi=1.2)
    return _override(p, 'push_route_params', overrides)


def depth_noise_params(config=None, **overrides):
    """The ``rv_depth_noise_params`` of an ``OBSERVATION.DEPTH_NOISE`` config: a mapping with the keys GAMMA_SHAPE, PROB,
    RESCALE_FACTOR, SIGMA, SEED (any of them may be missing: the defaults are those of the reference's ``gamma_noise`` /
    ``gaussian_noise``: 1000, 0.5, 4, 0.005, and seed 0).  ``height`` / ``width`` / ``draw_index`` start at 0 -- ``World.
    depth_noise`` fills the size in from the tensor -- and keyword arguments override fields by their C names.  A
    RESCALE_FACTOR that is not an integer becomes -1, which the library refuses."""
    cfg = dict(config or {})
    unknown = set(cfg) - {'GAMMA_SHAPE', 'PROB', 'RESCALE_FACTOR', 'SIGMA', 'SEED'}
    if unknown:
        raise TypeError('depth_noise_params: unknown keys %s' % (sorted(unknown),))
    r = cfg.get('RESCALE_FACTOR', 4)
    p = abi.rv_depth_noise_params(height=0, width=0, draw_index=0, seed=int(cfg.get('SEED', 0)) & 0xFFFFFFFF,
                                  gamma_shape=float(cfg.get('GAMMA_SHAPE', 1000.0)), prob=float(cfg.get('PROB', 0.5)),
                                  rescale_factor=int(r) if float(r) == int(r) else -1, sigma=float(cfg.get('SIGMA', 0.005)))
    return _override(p, 'depth_noise_params', overrides)


def segment_params(num_points=256, num_clusters=abi.RV_MAXB, **overrides):
    """An ``rv_segment_params`` with the reference's constants: 50 plane hypotheses (PCL's default iteration count, as
    recalled), plane_thresh 0.015 (``remove_table``), eps 0.02 and min_samples 50 (``cluster(method='dbscan')``),
    ``num_clusters`` slots of ``num_points`` points, draw_index 0.  Keyword arguments override fields by their C names."""
    p = abi.rv_segment_params(num_hypotheses=50, plane_thresh=0.015, eps=0.02, min_samples=50, num_clusters=int(num_clusters),
                              num_points=int(num_points), draw_index=0)
    return _override(p, 'segment_params', overrides)


def ward_params(num_points=256, num_groups=abi.RV_MAXB, num_neighbors=100, **overrides):
    """An ``rv_ward_params`` with the reference's constant: the 100 nearest neighbours of its second ``cluster()`` call,
    ``num_groups`` slots of ``num_points`` points, draw_index 0.  Keyword arguments override fields by their C names."""
    p = abi.rv_ward_params(num_neighbors=int(num_neighbors), num_groups=int(num_groups), num_points=int(num_points), draw_index=0)
    return _override(p, 'ward_params', overrides)


def grasp_crop_params(crop_height=32, crop_width=32, step=3, **overrides):
    """An ``rv_grasp_crop_params``: ``crop_height`` x ``crop_width`` output pixels, every ``step``-th pixel of a window of
    ``step`` times that size around the grasp.  The defaults are BUILD-CHOSEN, not the reference's (its ``transform`` and
    ``crop`` take their sizes from the caller): a 96-pixel window sampled to 32 x 32.  ``height`` / ``width`` start at 0
    -- ``World.grasp_crops`` fills them in from the tensor -- and keyword arguments override fields by their C names."""
    p = abi.rv_grasp_crop_params(height=0, width=0, crop_height=int(crop_height), crop_width=int(crop_width), step=int(step))
    return _override(p, 'grasp_crop_params', overrides)


def grasp_refine_params(n_elites=1, sigma_center=3.0, sigma_angle=0.15, sigma_depth=0.005, macro_index=0, iteration=0,
                        seed=0, **overrides):
    """An ``rv_grasp_refine_params``: ``n_elites`` kept rows, the standard deviations of a child's centre (pixels), axis
    angle (radians) and depth (metres), and the Philox arguments ``macro_index`` (the env.step() being chosen),
    ``iteration`` (the refinement round) and ``seed``.  The default sigmas are BUILD-CHOSEN and unmeasured.
    ``height`` / ``width`` start at 0 -- ``World.grasp_refine`` fills them in from the tensor -- and keyword arguments
    override fields by their C names."""
    p = abi.rv_grasp_refine_params(height=0, width=0, macro_index=int(macro_index), iteration=int(iteration),
                                   seed=int(seed) & 0xFFFFFFFF, n_elites=int(n_elites), sigma_center=float(sigma_center),
                                   sigma_angle=float(sigma_angle), sigma_depth=float(sigma_depth))
    return _override(p, 'grasp_refine_params', overrides)


def adam_params(step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """An ``rv_adam_params`` for update number ``step`` (t >= 1): lr, the betas and eps rounded to float32, and the bias
    corrections 1 / (1 - beta^t) computed in float64 from the float32 betas and rounded once."""
    import numpy as np
    step = int(step)
    if step < 1:
        raise ValueError('adam_params: step must be >= 1, got %d' % step)
    b1, b2 = float(np.float32(betas[0])), float(np.float32(betas[1]))
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError('adam_params: betas outside [0, 1): %r' % (betas,))
    return abi.rv_adam_params(lr=float(lr), beta1=b1, beta2=b2, eps=float(eps), corr1=1.0 / (1.0 - b1 ** step),
                              corr2=1.0 / (1.0 - b2 ** step))


def view_params(n_views, height, width, supersample=1):
    """An ``rv_view_params`` for ``rv_render_view``: ``n_views`` images of ``height`` x ``width`` pixels, ``supersample`` x
    ``supersample`` rays per rgb pixel.  ValueError for what the library refuses as well: a count outside [1,
    abi.RV_VIEW_MAX_VIEWS], a side outside [1, abi.RV_VIEW_MAX_SIDE], a supersample outside [1,
    abi.RV_VIEW_MAX_SUPERSAMPLE], or a value that is not an integer."""
    vals = {}
    for name, v, hi in (('n_views', n_views, abi.RV_VIEW_MAX_VIEWS), ('height', height, abi.RV_VIEW_MAX_SIDE),
                        ('width', width, abi.RV_VIEW_MAX_SIDE), ('supersample', supersample, abi.RV_VIEW_MAX_SUPERSAMPLE)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError('view_params: %s must be an integer, got %r' % (name, v))
        if not 1 <= int(v) <= hi:
            raise ValueError('view_params: %s = %d outside [1, %d]' % (name, int(v), hi))
        vals[name] = int(v)
    return abi.rv_view_params(**vals)


def check(status):
    if status != abi.RV_OK:
        msg = load().rv_last_error().decode('utf-8', 'replace')
        raise _EXC.get(status, RuntimeError)(msg)


class Snapshot(object):
    """The env blocks of a world at one moment (``World.save_state``): ``blocks`` is a torch uint8 tensor [N, bytes] on
    the world's device, ``source_hash`` the hash of the sources the library that wrote them was built from, and
    ``config_key`` the rv_config bytes a world must share to take them (``abi.config_key``: all but n_envs and
    env_id_offset).  It lives in device memory and only as long as the process: blocks mean nothing to another build."""

    def __init__(self, blocks, source_hash, config_key):
        self.blocks = blocks
        self.source_hash = source_hash
        self.config_key = config_key

    @property
    def n_blocks(self):
        return int(self.blocks.shape[0])


class World(object):
    """N batched envs on one GPU.  Buffers are torch tensors on that device;
    the C ABI only ever sees their raw ``data_ptr()``."""

    def __init__(self, cfg, scene, device=0):
        import torch
        self.torch = torch
        self.lib = load()
        self.cfg = cfg
        self.scene = scene
        self.n = int(cfg.n_envs)
        self.G = cfg.num_goal_steps if cfg.num_goal_steps > 0 else 1
        self.device_index = int(device)
        self.device = torch.device('cuda', self.device_index)
        self.h = C.c_void_p()
        self._ward_workspace = None      # (ward_groups: int64 words, grown on demand)
        check(self.lib.rv_create(C.byref(cfg), C.byref(scene), self.device_index, C.byref(self.h)))
        # run on torch's current stream so torch ops and kernels are ordered
        self.use_current_stream()

    def use_current_stream(self):
        stream = self.torch.cuda.current_stream(self.device)
        check(self.lib.rv_set_stream(self.h, C.c_void_p(stream.cuda_stream)))

    def close(self):
        if getattr(self, 'h', None) and self.h:
            self.lib.rv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers
    def _new(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device=self.device)

    def _in(self, x, shape, dtype):
        t = self.torch.as_tensor(x, dtype=dtype, device=self.device).reshape(shape).contiguous()
        return t

    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr())

    def synchronize(self):
        check(self.lib.rv_synchronize(self.h))

    def env_kernel_build(self):
        """rv_env_kernel_build: abi.RV_ENV_BUILD_OCC1 (k_env) or abi.RV_ENV_BUILD_OCC2 (k_env_occ2), as rv_create chose."""
        return int(self.lib.rv_env_kernel_build(self.h))

    # -- env stepping
    def reset(self, mask=None):
        if mask is None:
            check(self.lib.rv_reset(self.h, None))
        else:
            m = self._in(mask, (self.n,), self.torch.uint8)
            check(self.lib.rv_reset(self.h, self._ptr(m)))

    def set_actions(self, actions):
        a = self._in(actions, (self.n, self.G, 4), self.torch.float32)
        check(self.lib.rv_set_actions(self.h, self._ptr(a)))

    def step_macro(self):
        check(self.lib.rv_step_macro(self.h))

    def step_begin(self, actions, mask=None):
        """rv_step_begin: the next action of the envs flagged in ``mask`` (uint8 [N], None = all)."""
        a = self._in(actions, (self.n, self.G, 4), self.torch.float32)
        m = None if mask is None else self._in(mask, (self.n,), self.torch.uint8)
        check(self.lib.rv_step_begin(self.h, self._ptr(a), None if m is None else self._ptr(m)))

    def set_auto_reset(self, on=True):
        """rv_set_auto_reset: step_begin on a finished episode resets the env; the next poll returns the reset observation."""
        check(self.lib.rv_set_auto_reset(self.h, int(bool(on))))

    def step_poll(self, max_substeps=0, max_usec=0, out=None):
        """rv_step_poll: advance the stepping envs within the budget; returns uint8 [N], 1 = this
        env's env.step() completed in this launch.  ``out`` (from ``poll_buffers``): the observation,
        reward and done of the envs that finished are written to their rows."""
        f = self._new((self.n,), self.torch.uint8)
        if out is None:
            check(self.lib.rv_step_poll(self.h, int(max_substeps), int(max_usec), self._ptr(f), None, None, None))
        else:
            check(self.lib.rv_step_poll(self.h, int(max_substeps), int(max_usec), self._ptr(f), C.byref(out['_buffers']),
                                        self._ptr(out['reward']), self._ptr(out['done'])))
        return f

    def poll_buffers(self, point_cloud=True, pose_modes=False):
        """Persistent [N]-row buffers for ``step_poll(out=...)``: {'obs': dict, 'reward', 'done'}."""
        obs, b = self._obs_buffers((self.n,), point_cloud, pose_modes)
        return {'obs': obs, '_buffers': b, 'reward': self.torch.zeros((self.n,), dtype=self.torch.float32, device=self.device),
                'done': self.torch.zeros((self.n,), dtype=self.torch.uint8, device=self.device)}

    def rollout(self, n_steps, first_macro_index=0, auto_reset=True, record=False):
        """n_steps x (RandomPolicy action -> env.step) per env in one launch."""
        r = d = None
        if record:
            r = self.torch.zeros((int(n_steps), self.n), dtype=self.torch.float32, device=self.device)
            d = self.torch.ones((int(n_steps), self.n), dtype=self.torch.uint8, device=self.device)
        check(self.lib.rv_rollout(self.h, int(n_steps), int(first_macro_index), int(bool(auto_reset)),
                                  self._ptr(r) if record else None, self._ptr(d) if record else None))
        return r, d

    def _obs_buffers(self, lead, point_cloud, pose_modes):
        """Zeroed observation tensors with leading shape ``lead`` + the rv_obs_buffers of their pointers."""
        t = self.torch

        def z(shape, dtype):
            return t.zeros(tuple(lead) + shape, dtype=dtype, device=self.device)
        out = {
            'position': z((abi.RV_MAXB, 3), t.float32), 'body_mask': z((abi.RV_MAXB,), t.float32),
            'num_episodes': z((), t.int64), 'num_steps': z((), t.int64), 'layout_id': z((), t.int64),
            'is_safe': z((), t.int64), 'is_effective': z((), t.int64),
        }
        b = abi.rv_obs_buffers()
        b.d_position = out['position'].data_ptr(); b.d_body_mask = out['body_mask'].data_ptr()
        b.d_num_episodes = out['num_episodes'].data_ptr(); b.d_num_steps = out['num_steps'].data_ptr()
        b.d_layout_id = out['layout_id'].data_ptr(); b.d_is_safe = out['is_safe'].data_ptr()
        b.d_is_effective = out['is_effective'].data_ptr()
        if point_cloud:
            out['point_cloud'] = z((abi.RV_MAXB, int(self.cfg.num_points), 3), t.float32)
            b.d_point_cloud = out['point_cloud'].data_ptr()
        if pose_modes:      # the other PoseObs modalities (pose_obs.py:53-73)
            out['pose'] = z((abi.RV_MAXB, 6), t.float32)
            out['pose2d'] = z((abi.RV_MAXB, 3), t.float32)
            out['yaw_cossin'] = z((abi.RV_MAXB, 2), t.float32)
            b.d_pose = out['pose'].data_ptr(); b.d_pose2d = out['pose2d'].data_ptr()
            b.d_yaw_cossin = out['yaw_cossin'].data_ptr()
        return out, b

    def rollout_record(self, n_steps, first_macro_index=0, auto_reset=True, point_cloud=True, pose_modes=False):
        """The rollout returning what every env.step() returns: per-step observation rows
        [n_steps, N, ...], rewards and dones (rv_rollout_record)."""
        k = int(n_steps)
        obs, b = self._obs_buffers((k, self.n), point_cloud, pose_modes)
        r = self.torch.zeros((k, self.n), dtype=self.torch.float32, device=self.device)
        d = self.torch.ones((k, self.n), dtype=self.torch.uint8, device=self.device)
        check(self.lib.rv_rollout_record(self.h, k, int(first_macro_index), int(bool(auto_reset)),
                                         self._ptr(r), self._ptr(d), C.byref(b)))
        return obs, r, d

    def rollout_record_full(self, n_steps, first_macro_index=0, auto_reset=True, point_cloud=True, pose_modes=False):
        """rollout_record plus what a complete episode record needs (rv_rollout_record_full): returns
        (obs, rewards, dones, extra) with extra = {'actions' [K, N, G, 4], 'reset' [K, N] uint8,
        'reset_obs' dict of [K, N, ...] observations env.reset() returned before the steps that
        an auto-reset preceded (zero rows elsewhere)}; feed io.hdf5_utils.episodes_from_rollout."""
        k = int(n_steps)
        obs, b = self._obs_buffers((k, self.n), point_cloud, pose_modes)
        robs, rb = self._obs_buffers((k, self.n), point_cloud, pose_modes)
        r = self.torch.zeros((k, self.n), dtype=self.torch.float32, device=self.device)
        d = self.torch.ones((k, self.n), dtype=self.torch.uint8, device=self.device)
        acts = self.torch.zeros((k, self.n, self.G, 4), dtype=self.torch.float32, device=self.device)
        rst = self.torch.zeros((k, self.n), dtype=self.torch.uint8, device=self.device)
        ex = abi.rv_rollout_extra()
        ex.d_actions = acts.data_ptr(); ex.d_reset = rst.data_ptr(); ex.reset_obs = rb
        check(self.lib.rv_rollout_record_full(self.h, k, int(first_macro_index), int(bool(auto_reset)),
                                              self._ptr(r), self._ptr(d), C.byref(b), C.byref(ex)))
        return obs, r, d, {'actions': acts, 'reset': rst, 'reset_obs': robs}

    def last_tail_renders(self):
        """rv_last_tail_renders: (by_tail, by_residual) -- the snapshot rows of the last recorded rollout whose point
        clouds the rollout kernel's finished workgroups rendered / the launch after the kernel rendered."""
        a, b = C.c_int32(0), C.c_int32(0)
        check(self.lib.rv_last_tail_renders(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def rollout_async(self, total_env_steps, first_macro_index=0):
        """total_env_steps x (RandomPolicy action -> env.step) shared by all envs: every env
        keeps stepping (auto-reset) while the pool lasts.  Returns steps taken per env."""
        taken = self._new((self.n,), self.torch.int32)
        check(self.lib.rv_rollout_async(self.h, int(total_env_steps), int(first_macro_index), self._ptr(taken)))
        return taken

    def step_sub(self, n):
        check(self.lib.rv_step_sub(self.h, int(n)))

    def wait_until_stable(self, lin=0.005, ang=0.005, check_after=100, min_stable=100, max_steps=2000):
        check(self.lib.rv_wait_until_stable(self.h, lin, ang, check_after, min_stable, max_steps))

    def policy_random(self, macro_index):
        a = self._new((self.n, self.G, 4), self.torch.float32)
        check(self.lib.rv_policy_random(self.h, int(macro_index), self._ptr(a)))
        return a

    def policy_heuristic(self, max_attempts=20000):
        a = self._new((self.n, self.G, 4), self.torch.float32)
        check(self.lib.rv_policy_heuristic(self.h, int(max_attempts), self._ptr(a)))
        return a

    def policy_antipodal(self, params, macro_index, depth=None, actions4=True):
        """rv_policy_antipodal: AntipodalGrasp4DofPolicy for every env.  ``params``: an ``abi.rv_antipodal_params``
        (``antipodal_params(config)``); ``depth`` [N, H, W] on the device (None: rendered now).  Returns
        (image grasps [N, 5], 4-DoF actions [N, 4] or None, status int32 [N])."""
        g = self._new((self.n, 5), self.torch.float32)
        st = self._new((self.n,), self.torch.int32)
        a = self._new((self.n, 4), self.torch.float32) if actions4 else None
        d = None
        if depth is not None:
            d = self._in(depth, (self.n, int(self.cfg.cam_height), int(self.cfg.cam_width)), self.torch.float32)
        check(self.lib.rv_policy_antipodal(self.h, None if d is None else self._ptr(d), C.byref(params), int(macro_index),
                                           self._ptr(g), None if a is None else self._ptr(a), self._ptr(st)))
        return g, a, st

    def policy_antipodal_multi(self, params, macro_index, num_samples, depth=None, actions4=True):
        """rv_policy_antipodal_multi: up to ``num_samples`` (K) distinct antipodal grasps for every env, the reference's
        ``sample(depth, camera, K)``.  Arguments as ``policy_antipodal``.  Returns (image grasps [N, K, 5], 4-DoF
        actions [N, K, 4] or None, count int32 [N], status int32 [N]); rows from ``count`` on repeat row 0, and row 0
        is the grasp ``policy_antipodal`` returns."""
        k = int(num_samples)
        rows = min(max(k, 1), abi.RV_AP_MAX_SAMPLES)      # (the library refuses a K outside [1, RV_AP_MAX_SAMPLES])
        g = self._new((self.n, rows, 5), self.torch.float32)
        cnt = self._new((self.n,), self.torch.int32)
        st = self._new((self.n,), self.torch.int32)
        a = self._new((self.n, rows, 4), self.torch.float32) if actions4 else None
        d = None
        if depth is not None:
            d = self._in(depth, (self.n, int(self.cfg.cam_height), int(self.cfg.cam_width)), self.torch.float32)
        check(self.lib.rv_policy_antipodal_multi(self.h, None if d is None else self._ptr(d), C.byref(params), int(macro_index), k,
                                                 self._ptr(g), None if a is None else self._ptr(a), self._ptr(cnt), self._ptr(st)))
        return g, a, cnt, st

    def _plan_in(self, x, tail):
        """float32, contiguous, on the device and 16-byte aligned (the kernels read a [4][2] record as two float4);
        a trailing z column ([..., 3] positions) is dropped"""
        t = self.torch.as_tensor(x, dtype=self.torch.float32, device=self.device)
        if t.dim() >= 1 and t.shape[-1] == 3:
            t = t[..., :2]
        if tuple(t.shape[t.dim() - len(tail):]) != tuple(tail):
            raise ValueError('expected [..., %s] positions, got %s' % (', '.join(str(v) for v in tail), tuple(t.shape)))
        t = t.contiguous()
        return t.clone() if t.data_ptr() % 16 else t

    def plan_reward(self, state, next_state, params=None):
        """rv_plan_reward: planning-mode PushReward of M transitions, ``state`` / ``next_state`` [M, B, 2] (or
        [M, B, 3]; B from the tensor unless ``params`` is given).  Returns (reward float32 [M], termination uint8 [M])."""
        s = self.torch.as_tensor(state)
        if s.dim() != 3:
            raise ValueError('plan_reward: state must be [M, B, 2]')
        m, b = int(s.shape[0]), int(s.shape[1])
        p = params if params is not None else plan_params(n_bodies=b)
        s = self._plan_in(s, (b, 2)); nx = self._plan_in(next_state, (b, 2))
        if tuple(nx.shape) != tuple(s.shape) or int(p.n_bodies) != b:
            raise ValueError('plan_reward: state, next_state and params.n_bodies disagree')
        r = self._new((m,), self.torch.float32)
        t = self._new((m,), self.torch.uint8)
        check(self.lib.rv_plan_reward(self.h, C.byref(p), self._ptr(s), self._ptr(nx), m, self._ptr(r), self._ptr(t)))
        return r, t

    def plan_score(self, plans, state0=None, params=None):
        """rv_plan_score: ``plans`` [N, S, H, B, 2] (or [..., 3]) are the states after each step of S candidate plans
        per env, ``state0`` [N, B, 2] the state before the first (None: the xy of the env's last observation).
        Returns (returns float32 [N, S], lengths int32 [N, S], best int32 [N])."""
        pl = self.torch.as_tensor(plans)
        if pl.dim() != 5 or int(pl.shape[0]) != self.n:
            raise ValueError('plan_score: plans must be [N, S, H, B, 2] with N = %d' % self.n)
        s, h, b = int(pl.shape[1]), int(pl.shape[2]), int(pl.shape[3])
        p = params if params is not None else plan_params(n_bodies=b)
        if int(p.n_bodies) != b:
            raise ValueError('plan_score: plans and params.n_bodies disagree')
        pl = self._plan_in(pl, (b, 2))
        s0 = None if state0 is None else self._plan_in(state0, (b, 2)).reshape(self.n, b, 2)
        ret = self._new((self.n, s), self.torch.float32)
        ln = self._new((self.n, s), self.torch.int32)
        best = self._new((self.n,), self.torch.int32)
        check(self.lib.rv_plan_score(self.h, C.byref(p), None if s0 is None else self._ptr(s0), self._ptr(pl), s, h,
                                     self._ptr(ret), self._ptr(ln), self._ptr(best)))
        return ret, ln, best

    # -- the cross-entropy-method planner's two kernels (include/rovat.h: rv_cem_sample / rv_cem_refit)
    def _cem_dist(self, who, mean, std):
        """mean and std as float32 [N, D] on the device, D from the tensors"""
        m = self.torch.as_tensor(mean, dtype=self.torch.float32, device=self.device)
        sd = self.torch.as_tensor(std, dtype=self.torch.float32, device=self.device)
        if m.dim() < 2 or int(m.shape[0]) != self.n or tuple(sd.shape) != tuple(m.shape):
            raise ValueError('%s: mean and std must both be [N, ...] with N = %d' % (who, self.n))
        return m.reshape(self.n, -1).contiguous(), sd.reshape(self.n, -1).contiguous()

    def cem_sample(self, mean, std, params, s, h):
        """rv_cem_sample: ``s`` candidate plans of ``h`` steps per env from the normal distribution ``mean`` / ``std``
        ([N, h * G * 4], or any [N, ...] of that many floats), clamped to [-1, 1].  ``params``: ``cem_params(...)``.
        Returns float32 [N, s, h, G, 4], what ``plan_simulate`` takes."""
        s, h = int(s), int(h)
        m, sd = self._cem_dist('cem_sample', mean, std)
        if int(m.shape[1]) != h * self.G * 4:
            raise ValueError('cem_sample: mean and std must hold h * G * 4 = %d floats per env, got %d' % (h * self.G * 4, int(m.shape[1])))
        rows = min(max(s, 1), abi.RV_CEM_MAX_SAMPLES)      # (the library refuses an s outside [1, RV_CEM_MAX_SAMPLES])
        a = self._new((self.n, rows, max(h, 1), self.G, 4), self.torch.float32)
        check(self.lib.rv_cem_sample(self.h, C.byref(params), self._ptr(m), self._ptr(sd), s, h, self._ptr(a)))
        return a

    def cem_refit(self, actions, returns, mean, std, params, elite=True):
        """rv_cem_refit: rank the candidates ``actions`` [N, S, H, G, 4] by ``returns`` [N, S] and fit ``mean`` /
        ``std`` ([N, H * G * 4], or any [N, ...] of that many floats) to the first ``params.n_elites``.  The arguments
        stay as they are.  Returns (mean, std -- new tensors in the shape given --, elite int32 [N, E] by rank, or None
        with ``elite=False``)."""
        a = self.torch.as_tensor(actions, dtype=self.torch.float32, device=self.device)
        if a.dim() == 4 and self.G == 1:
            a = a[:, :, :, None]
        if a.dim() != 5 or int(a.shape[0]) != self.n or tuple(a.shape[3:]) != (self.G, 4):
            raise ValueError('cem_refit: actions must be [N, S, H, %d, 4] with N = %d, got %s' % (self.G, self.n, tuple(a.shape)))
        s, h = int(a.shape[1]), int(a.shape[2])
        r = self.torch.as_tensor(returns, dtype=self.torch.float32, device=self.device)
        if tuple(r.shape) != (self.n, s):
            raise ValueError('cem_refit: returns must be [N, S] = [%d, %d], got %s' % (self.n, s, tuple(r.shape)))
        m, sd = self._cem_dist('cem_refit', mean, std)
        if int(m.shape[1]) != h * self.G * 4:
            raise ValueError('cem_refit: mean and std must hold H * G * 4 = %d floats per env, got %d' % (h * self.G * 4, int(m.shape[1])))
        shape = tuple(self.torch.as_tensor(mean).shape)
        m, sd = m.clone(), sd.clone()      # (the kernel updates in place)
        a, r = a.contiguous(), r.contiguous()
        e = int(params.n_elites)
        el = self._new((self.n, min(max(e, 1), max(s, 1))), self.torch.int32) if elite else None
        check(self.lib.rv_cem_refit(self.h, C.byref(params), self._ptr(a), self._ptr(r), s, h,
                                    self._ptr(m), self._ptr(sd), None if el is None else self._ptr(el)))
        return m.reshape(shape), sd.reshape(shape), el

    # -- the depth sensor noise model (include/rovat.h: rv_depth_noise)
    def depth_noise(self, depth, params, out=None, record=False):
        """rv_depth_noise: the gamma multiplier and the upsampled Gaussian grid of ``params`` (``depth_noise_params(...)``;
        its height and width are taken from the tensor) on ``depth``, float32 [N, H, W] on the device.  ``out``: None for a
        new tensor, or a float32 [N, H, W] tensor to write (``depth`` itself: in place).  Returns the noisy depth, or with
        ``record=True`` (noisy depth, g float32 [N], applied uint8 [N], grid float32 [N, H / R, W / R]) -- the grid of an
        env the noise was not applied to, and every grid with sigma 0, reads zero."""
        torch = self.torch
        d = torch.as_tensor(depth, dtype=torch.float32, device=self.device)
        if d.dim() != 3 or int(d.shape[0]) != self.n:
            raise ValueError('depth_noise: depth must be [N, H, W] with N = %d, got %s' % (self.n, tuple(d.shape)))
        d = d.contiguous()
        if out is None:
            out = self._new(tuple(d.shape), torch.float32)
        elif not (torch.is_tensor(out) and out.dtype == torch.float32 and out.device == d.device
                  and tuple(out.shape) == tuple(d.shape) and out.is_contiguous()):
            raise ValueError('depth_noise: out must be a contiguous float32 tensor like depth, on its device')
        p = abi.rv_depth_noise_params.from_buffer_copy(params)
        p.height, p.width = int(d.shape[1]), int(d.shape[2])
        g = ap = grid = None
        if record:
            r = int(p.rescale_factor) if 1 <= int(p.rescale_factor) <= abi.RV_DN_MAX_RESCALE else 1
            g = self._new((self.n,), torch.float32)
            ap = self._new((self.n,), torch.uint8)
            grid = torch.zeros((self.n, p.height // r, p.width // r), dtype=torch.float32, device=self.device)
        check(self.lib.rv_depth_noise(self.h, C.byref(p), self._ptr(d), self._ptr(out), None if g is None else self._ptr(g),
                                      None if ap is None else self._ptr(ap), None if grid is None else self._ptr(grid)))
        return (out, g, ap, grid) if record else out

    # -- point clouds segmented without the segmask (include/rovat.h: rv_deproject / rv_segment_cloud)
    def deproject(self, depth, env_first=0):
        """rv_deproject: ``depth`` float32 [n, H, W] (the camera's size) of the envs ``env_first`` .. ``env_first + n - 1``
        through each env's own calibration.  Returns (points float32 [n, H * W, 3], valid uint8 [n, H * W]: depth > 0 and
        inside the config's crop)."""
        torch = self.torch
        h, w = int(self.cfg.cam_height), int(self.cfg.cam_width)
        d = torch.as_tensor(depth, dtype=torch.float32, device=self.device)
        if d.dim() != 3 or tuple(d.shape[1:]) != (h, w):
            raise ValueError('deproject: depth must be [n, %d, %d], got %s' % (h, w, tuple(d.shape)))
        d = d.contiguous()
        n = int(d.shape[0])
        pts = self._new((n, h * w, 3), torch.float32)
        valid = self._new((n, h * w), torch.uint8)
        check(self.lib.rv_deproject(self.h, int(env_first), n, self._ptr(d), self._ptr(pts), self._ptr(valid)))
        return pts, valid

    def segment_cloud(self, points, valid, params, env_first=0):
        """rv_segment_cloud: ``points`` float32 [n, M, 3] and ``valid`` uint8 [n, M] (or None: all valid) of the envs
        ``env_first`` .. ``env_first + n - 1``; ``params``: ``segment_params(...)``.  Returns a dict of device tensors:
        clouds float32 [n, C, P, 3], labels int32 [n, M], slot_labels / slot_counts int32 [n, C], plane float32 [n, 4], info
        int32 [n, 8] (abi.RV_SEG_INFO_*)."""
        torch = self.torch
        pts = torch.as_tensor(points, dtype=torch.float32, device=self.device)
        if pts.dim() != 3 or int(pts.shape[2]) != 3:
            raise ValueError('segment_cloud: points must be [n, M, 3], got %s' % (tuple(pts.shape),))
        pts = pts.contiguous()
        n, m = int(pts.shape[0]), int(pts.shape[1])
        v = None
        if valid is not None:
            v = torch.as_tensor(valid, device=self.device)
            if tuple(v.shape) != (n, m):
                raise ValueError('segment_cloud: valid must be [n, M] = [%d, %d], got %s' % (n, m, tuple(v.shape)))
            v = v.to(torch.uint8).contiguous()
        c = min(max(int(params.num_clusters), 1), abi.RV_SEG_MAXSLOTS)      # (the library refuses what is outside)
        p = min(max(int(params.num_points), 1), abi.RV_SEG_MAX_POINTS)
        out = dict(clouds=self._new((n, c, p, 3), torch.float32), labels=self._new((n, max(m, 1)), torch.int32),
                   slot_labels=self._new((n, c), torch.int32), slot_counts=self._new((n, c), torch.int32),
                   plane=self._new((n, 4), torch.float32), info=self._new((n, abi.RV_SEG_INFO_WORDS), torch.int32))
        check(self.lib.rv_segment_cloud(self.h, C.byref(params), int(env_first), n, self._ptr(pts), None if v is None else self._ptr(v),
                                        m, self._ptr(out['labels']), self._ptr(out['clouds']), self._ptr(out['slot_labels']),
                                        self._ptr(out['slot_counts']), self._ptr(out['plane']), self._ptr(out['info'])))
        return out

    def ward_groups(self, points, labels, params, env_first=0):
        """rv_ward_groups: ``points`` float32 [n, M, 3] and ``labels`` int32 [n, M] (``segment_cloud``'s) of the envs
        ``env_first`` .. ``env_first + n - 1``; ``params``: ``ward_params(...)``.  The points with a label >= 0 are
        agglomerated into exactly C groups.  Returns a dict of device tensors: clouds float32 [n, C, P, 3],
        groups int32 [n, M], slot_counts int32 [n, C], info int32 [n, 8] (abi.RV_WARD_INFO_*).  The workspace belongs to
        the world: allocated on the first call, grown when a larger chunk comes."""
        torch = self.torch
        pts = torch.as_tensor(points, dtype=torch.float32, device=self.device)
        if pts.dim() != 3 or int(pts.shape[2]) != 3:
            raise ValueError('ward_groups: points must be [n, M, 3], got %s' % (tuple(pts.shape),))
        pts = pts.contiguous()
        n, m = int(pts.shape[0]), int(pts.shape[1])
        lab = torch.as_tensor(labels, device=self.device)
        if tuple(lab.shape) != (n, m):
            raise ValueError('ward_groups: labels must be [n, M] = [%d, %d], got %s' % (n, m, tuple(lab.shape)))
        lab = lab.to(torch.int32).contiguous()
        c = min(max(int(params.num_groups), 1), abi.RV_SEG_MAXSLOTS)      # (the library refuses what is outside)
        p = min(max(int(params.num_points), 1), abi.RV_SEG_MAX_POINTS)
        need = int(self.lib.rv_ward_workspace_bytes(n))
        ws = self._ward_workspace
        if ws is None or ws.numel() * 8 < need:
            ws = self._ward_workspace = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=self.device)
        out = dict(clouds=self._new((n, c, p, 3), torch.float32), groups=self._new((n, max(m, 1)), torch.int32),
                   slot_counts=self._new((n, c), torch.int32), info=self._new((n, abi.RV_WARD_INFO_WORDS), torch.int32))
        check(self.lib.rv_ward_groups(self.h, C.byref(params), int(env_first), n, self._ptr(pts), self._ptr(lab), m, self._ptr(ws),
                                      ws.numel() * 8, self._ptr(out['groups']), self._ptr(out['clouds']),
                                      self._ptr(out['slot_counts']), self._ptr(out['info'])))
        return out

    def clustered_point_cloud(self, params, chunk=256, depth=None, labels=False, ward=None):
        """render -> deproject -> segment_cloud for every env, ``chunk`` envs at a time so that the [chunk, H * W, 3] points
        stay bounded.  ``depth``: float32 [N, H, W] to segment instead of a fresh render (a noisy one, say).  Returns the dict
        of ``segment_cloud`` for all N envs (``labels`` [N, H * W] only when asked for).  ``ward``: ``ward_params(...)`` to
        chain ``ward_groups`` on every chunk: ``clouds`` and ``slot_counts`` are then its exactly-C groups, ``ward_info``
        [N, 8] is added, and ``groups`` [N, H * W] next to ``labels`` when those are asked for."""
        torch = self.torch
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError('clustered_point_cloud: chunk must be positive')
        if depth is None:
            depth, _ = self.render(segmask=False)
        parts = []
        for first in range(0, self.n, chunk):
            d = depth[first:first + chunk]
            pts, valid = self.deproject(d, env_first=first)
            r = self.segment_cloud(pts, valid, params, env_first=first)
            if ward is not None:
                g = self.ward_groups(pts, r['labels'], ward, env_first=first)
                r['clouds'], r['slot_counts'], r['ward_info'] = g['clouds'], g['slot_counts'], g['info']
                if labels:
                    r['groups'] = g['groups']
            if not labels:
                del r['labels']
            parts.append(r)
        return {k: torch.cat([r[k] for r in parts], dim=0) for k in parts[0]}

    # -- grasp-centred depth crops (include/rovat.h: rv_grasp_crops)
    def grasp_crops(self, depth, grasps, params, out=None, grasp_depths=True):
        """rv_grasp_crops: for every image grasp of ``grasps`` ([N, K, 5], or [N, 5] for K = 1: x1, y1, x2, y2, depth) the
        depth image of its env re-centred on the grasp, rotated so that the grasp axis is horizontal, and cropped to
        ``params`` (``grasp_crop_params(...)``; its height and width are taken from the tensor).  ``depth``: float32
        [N, H, W] on the device.  ``out``: None for a new tensor, or a contiguous float32 [N, K, h, w] tensor to write.
        Returns (images [N, K, h, w], grasp depths [N, K] -- column 4 of the rows -- or None with ``grasp_depths=False``)."""
        torch = self.torch
        d = torch.as_tensor(depth, dtype=torch.float32, device=self.device)
        if d.dim() != 3 or int(d.shape[0]) != self.n:
            raise ValueError('grasp_crops: depth must be [N, H, W] with N = %d, got %s' % (self.n, tuple(d.shape)))
        g = torch.as_tensor(grasps, dtype=torch.float32, device=self.device)
        if g.dim() == 2:
            g = g[:, None, :]
        if g.dim() != 3 or int(g.shape[0]) != self.n or int(g.shape[2]) != 5:
            raise ValueError('grasp_crops: grasps must be [N, K, 5] or [N, 5] with N = %d, got %s' % (self.n, tuple(g.shape)))
        d, g = d.contiguous(), g.contiguous()
        k = int(g.shape[1])
        p = abi.rv_grasp_crop_params.from_buffer_copy(params)
        p.height, p.width = int(d.shape[1]), int(d.shape[2])
        side = lambda v: min(max(int(v), 1), abi.RV_GC_MAX_SIDE)      # (the library refuses a size outside its range)
        shape = (self.n, min(max(k, 1), abi.RV_AP_MAX_SAMPLES), side(p.crop_height), side(p.crop_width))
        if out is None:
            out = self._new(shape, torch.float32)
        elif not (torch.is_tensor(out) and out.dtype == torch.float32 and out.device == d.device
                  and tuple(out.shape) == (self.n, k, int(p.crop_height), int(p.crop_width)) and out.is_contiguous()):
            raise ValueError('grasp_crops: out must be a contiguous float32 [N, K, h, w] tensor on the depth\'s device')
        gd = self._new((self.n, shape[1]), torch.float32) if grasp_depths else None
        check(self.lib.rv_grasp_crops(self.h, C.byref(p), self._ptr(d), self._ptr(g), k, self._ptr(out),
                                      None if gd is None else self._ptr(gd)))
        return out, gd

    # -- grasp-quality network (include/rovat.h: rv_grasp_quality)
    def grasp_quality(self, images, grasp_depths, model, out=None):
        """rv_grasp_quality: the logit of ``model`` (a ``perception.grasp_quality.GraspQualityModel``) for every crop.
        ``images``: float32 [N, K, h, w] with the model's h x w (or [N, h, w] for K = 1), as ``grasp_crops`` returns them;
        ``grasp_depths``: float32 [N, K] (or [N]); ``out``: None for a new tensor, or a contiguous float32 [N, K] tensor
        to write.  Returns the logits [N, K] (``torch.sigmoid`` makes probabilities of them).  The model's weight blob is
        uploaded once per model object and device and kept on the model."""
        torch = self.torch
        x = torch.as_tensor(images, dtype=torch.float32, device=self.device)
        if x.dim() == 3:
            x = x[:, None]
        h, w = int(model.sizes['height']), int(model.sizes['width'])
        if x.dim() != 4 or int(x.shape[0]) != self.n or tuple(x.shape[2:]) != (h, w):
            raise ValueError('grasp_quality: images must be [N, K, %d, %d] with N = %d, got %s' % (h, w, self.n, tuple(x.shape)))
        k = int(x.shape[1])
        z = torch.as_tensor(grasp_depths, dtype=torch.float32, device=self.device)
        if z.dim() == 1:
            z = z[:, None]
        if tuple(z.shape) != (self.n, k):
            raise ValueError('grasp_quality: grasp_depths must be [N, K] = [%d, %d], got %s' % (self.n, k, tuple(z.shape)))
        x, z = x.contiguous(), z.contiguous()
        if out is None:
            out = self._new((self.n, min(max(k, 1), abi.RV_AP_MAX_SAMPLES)), torch.float32)
        elif not (torch.is_tensor(out) and out.dtype == torch.float32 and out.device == x.device
                  and tuple(out.shape) == (self.n, k) and out.is_contiguous()):
            raise ValueError('grasp_quality: out must be a contiguous float32 [N, K] tensor on the images\' device')
        key = str(self.device)
        blob = model._device_blobs.get(key)
        if blob is None:
            desc = model.descriptor()
            count = int(self.lib.rv_grasp_quality_weight_count(C.byref(desc)))
            host = model.blob()
            if count != host.size:
                raise ValueError('grasp_quality: the library wants %d weights for this model, blob() has %d' % (count, host.size))
            blob = model._device_blobs[key] = torch.from_numpy(host).to(self.device)
        desc = model.descriptor()
        check(self.lib.rv_grasp_quality(self.h, C.byref(desc), self._ptr(blob), self._ptr(x), self._ptr(z), k, self._ptr(out)))
        return out

    # -- a training step of the grasp-quality network (include/rovat.h: rv_grasp_quality_forward_train, _backward, rv_adam_step)
    def _train_batch(self, who, model, images, grasp_depths):
        torch = self.torch
        h, w = int(model.sizes['height']), int(model.sizes['width'])
        x = torch.as_tensor(images, dtype=torch.float32, device=self.device)
        if x.dim() != 3 or tuple(x.shape[1:]) != (h, w) or not 1 <= int(x.shape[0]) <= abi.RV_GQ_MAX_BATCH:
            raise ValueError('%s: images must be [m, %d, %d] with m in [1, %d], got %s' % (who, h, w, abi.RV_GQ_MAX_BATCH, tuple(x.shape)))
        m = int(x.shape[0])
        z = torch.as_tensor(grasp_depths, dtype=torch.float32, device=self.device)
        if tuple(z.shape) != (m,):
            raise ValueError('%s: grasp_depths must be [m] = [%d], got %s' % (who, m, tuple(z.shape)))
        return x.contiguous(), z.contiguous(), m

    def _train_buffer(self, who, name, t, count, at_least=False):
        torch = self.torch
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == self.device and t.dim() == 1 and t.is_contiguous()
                and (int(t.numel()) >= count if at_least else int(t.numel()) == count)):
            raise ValueError('%s: %s must be a contiguous float32 tensor of %s%d floats on %s'
                             % (who, name, 'at least ' if at_least else '', count, self.device))
        return t

    def grasp_quality_train_workspace(self, model, m):
        """a new workspace tensor for ``m`` samples of ``model`` (rv_grasp_quality_train_workspace_floats)"""
        desc = model.descriptor()
        floats = int(self.lib.rv_grasp_quality_train_workspace_floats(C.byref(desc), int(m)))
        if floats < 0:
            raise ValueError('grasp_quality_train_workspace: the model or m = %d is refused' % (int(m),))
        return self._new((floats,), self.torch.float32)

    def grasp_quality_forward_train(self, model, weights, images, grasp_depths, workspace=None, out=None):
        """rv_grasp_quality_forward_train: the logits [m] of ``images`` [m, h, w] and ``grasp_depths`` [m] under the device
        blob ``weights`` (float32 [model.weight_count()], the layout of ``model.blob()``; ``model`` supplies the sizes and
        the normalisation only), bit for bit ``grasp_quality``'s, and the activations the backward pass reads in
        ``workspace`` (None: a new one).  Returns (logits, workspace).  Asynchronous."""
        who = 'grasp_quality_forward_train'
        x, z, m = self._train_batch(who, model, images, grasp_depths)
        desc = model.descriptor()
        wt = self._train_buffer(who, 'weights', weights, model.weight_count())
        need = int(self.lib.rv_grasp_quality_train_workspace_floats(C.byref(desc), m))
        if need < 0:
            raise ValueError('%s: the model is refused' % who)
        ws = self.grasp_quality_train_workspace(model, m) if workspace is None else self._train_buffer(who, 'workspace', workspace, need, True)
        out = self._new((m,), self.torch.float32) if out is None else self._train_buffer(who, 'out', out, m)
        check(self.lib.rv_grasp_quality_forward_train(self.h, C.byref(desc), self._ptr(wt), self._ptr(x), self._ptr(z), m,
                                                      self._ptr(ws), self._ptr(out)))
        return out, ws

    def grasp_quality_backward(self, model, weights, images, grasp_depths, dlogits, workspace, out=None):
        """rv_grasp_quality_backward: the gradient [model.weight_count()], in the blob's layout, of a loss whose derivative
        with respect to logit b is ``dlogits[b]``; ``workspace`` as ``grasp_quality_forward_train`` left it for the same
        weights, images and depths.  Deterministic: every entry is a float32 chain in a fixed order
        (csrc/rv_dev_grasp_train.h).  Asynchronous."""
        who = 'grasp_quality_backward'
        x, z, m = self._train_batch(who, model, images, grasp_depths)
        desc = model.descriptor()
        count = model.weight_count()
        wt = self._train_buffer(who, 'weights', weights, count)
        g = self._train_buffer(who, 'dlogits', dlogits, m)
        need = int(self.lib.rv_grasp_quality_train_workspace_floats(C.byref(desc), m))
        if need < 0:
            raise ValueError('%s: the model is refused' % who)
        ws = self._train_buffer(who, 'workspace', workspace, need, True)
        out = self._new((count,), self.torch.float32) if out is None else self._train_buffer(who, 'out', out, count)
        check(self.lib.rv_grasp_quality_backward(self.h, C.byref(desc), self._ptr(wt), self._ptr(x), self._ptr(z), self._ptr(g), m,
                                                 self._ptr(ws), self._ptr(out)))
        return out

    def adam_step(self, weights, grad, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        """rv_adam_step: one Adam update of ``weights`` in place from ``grad``, with the moments ``m`` and ``v`` (all float32
        [count] device tensors); ``step`` is t >= 1, the bias corrections 1 / (1 - beta^t) are computed here in float64."""
        count = int(weights.numel()) if self.torch.is_tensor(weights) else -1
        for name, t in (('weights', weights), ('grad', grad), ('m', m), ('v', v)):
            self._train_buffer('adam_step', name, t, count)
        check(self.lib.rv_adam_step(self.h, C.byref(adam_params(step, lr, betas, eps)), count, self._ptr(weights), self._ptr(grad),
                                    self._ptr(m), self._ptr(v)))
        return weights

    # -- cross-entropy refinement of grasp candidates (include/rovat.h: rv_grasp_refine)
    def grasp_refine(self, depth, grasps, scores, params, sampler_params, count=None, status=None, actions4=False):
        """rv_grasp_refine: the next generation of grasp candidates.  ``grasps`` [N, K, 5] are ranked per env by ``scores``
        [N, K]; the first ``params.n_elites`` stay, in rank order, and every further row is a child of an elite -- its centre,
        axis angle and depth perturbed by normals of ``params``' sigmas -- that passes the sampler's boundary and
        depth-window checks of ``sampler_params`` (``antipodal_params(config)``) on ``depth`` [N, H, W], or else its parent
        again.  ``count`` / ``status`` int32 [N]: the sampler's outputs (None: every row is a candidate).  ``params``:
        ``grasp_refine_params(...)``; its height and width are taken from the tensor.  Returns (grasps [N, K, 5], 4-DoF
        actions [N, K, 4] or None -- ``actions4=True`` needs a grasp world --, parent int32 [N, K]: the input row an output
        row came from, -1 - row for a child that fell back, count int32 [N]: K, or 0 for an env without a candidate)."""
        torch = self.torch
        d = torch.as_tensor(depth, dtype=torch.float32, device=self.device)
        if d.dim() != 3 or int(d.shape[0]) != self.n:
            raise ValueError('grasp_refine: depth must be [N, H, W] with N = %d, got %s' % (self.n, tuple(d.shape)))
        g = torch.as_tensor(grasps, dtype=torch.float32, device=self.device)
        if g.dim() != 3 or int(g.shape[0]) != self.n or int(g.shape[2]) != 5:
            raise ValueError('grasp_refine: grasps must be [N, K, 5] with N = %d, got %s' % (self.n, tuple(g.shape)))
        k = int(g.shape[1])
        s = torch.as_tensor(scores, dtype=torch.float32, device=self.device)
        if tuple(s.shape) != (self.n, k):
            raise ValueError('grasp_refine: scores must be [N, K] = [%d, %d], got %s' % (self.n, k, tuple(s.shape)))
        d, g, s = d.contiguous(), g.contiguous(), s.contiguous()
        cnt = st = None
        if count is not None:
            cnt = self._in(count, (self.n,), torch.int32)
        if status is not None:
            st = self._in(status, (self.n,), torch.int32)
        p = abi.rv_grasp_refine_params.from_buffer_copy(params)
        p.height, p.width = int(d.shape[1]), int(d.shape[2])
        rows = min(max(k, 1), abi.RV_AP_MAX_SAMPLES)      # (the library refuses a K outside [1, RV_AP_MAX_SAMPLES])
        out = self._new((self.n, rows, 5), torch.float32)
        a = self._new((self.n, rows, 4), torch.float32) if actions4 else None
        par = self._new((self.n, rows), torch.int32)
        cout = self._new((self.n,), torch.int32)
        opt = lambda t: None if t is None else self._ptr(t)
        check(self.lib.rv_grasp_refine(self.h, C.byref(p), C.byref(sampler_params), self._ptr(d), self._ptr(g), self._ptr(s),
                                       opt(cnt), opt(st), k, self._ptr(out), opt(a), self._ptr(par), self._ptr(cout)))
        return out, a, par, cout

    # -- env states as data (include/rovat.h: rv_state_* / rv_branch / rv_plan_simulate)
    def state_bytes(self):
        """rv_state_bytes: bytes of one env block of the loaded build."""
        return int(self.lib.rv_state_bytes(self.h))

    def save_state(self):
        """rv_state_save: a ``Snapshot`` of all N envs, asynchronous on the world's stream."""
        buf = self._new((self.n, self.state_bytes()), self.torch.uint8)
        check(self.lib.rv_state_save(self.h, self._ptr(buf)))
        return Snapshot(buf, built_source_hash(), abi.config_key(self.cfg))

    def load_state(self, snap, index=None):
        """rv_state_load: env j takes block ``index[j]`` of the snapshot (None: block j of a snapshot of N blocks; -1: env
        j stays as it is).  ValueError for a snapshot of another build or config and for an index outside
        [-1, n_blocks); no env changes then.  (Checking an index reads it back: one sync.)"""
        if not isinstance(snap, Snapshot):
            raise ValueError('load_state: not a Snapshot')
        if snap.source_hash != built_source_hash():
            raise ValueError('load_state: the snapshot was written by another build of the library')
        if snap.config_key != abi.config_key(self.cfg):
            raise ValueError('load_state: the snapshot comes from a world with another config')
        b = snap.blocks
        if (b.dim() != 2 or b.dtype != self.torch.uint8 or int(b.shape[1]) != self.state_bytes() or b.device != self.device
                or not b.is_contiguous()):
            raise ValueError('load_state: blocks must be a contiguous uint8 [n_blocks, %d] tensor on %s' % (self.state_bytes(), self.device))
        nb = snap.n_blocks
        if index is None:
            if nb != self.n:
                raise ValueError('load_state: a snapshot of %d blocks needs an index for a world of %d envs' % (nb, self.n))
            check(self.lib.rv_state_load(self.h, self._ptr(b), nb, None))
            return
        idx = self.torch.as_tensor(index, device=self.device)
        if idx.dtype.is_floating_point or idx.dtype == self.torch.bool or tuple(idx.shape) != (self.n,):
            raise ValueError('load_state: index must be %d integers' % self.n)
        if bool(((idx < -1) | (idx >= nb)).any()):
            raise ValueError('load_state: index outside [-1, %d)' % nb)
        idx = idx.to(self.torch.int32).contiguous()
        check(self.lib.rv_state_load(self.h, self._ptr(b), nb, self._ptr(idx)))

    def branch_from(self, src, s):
        """rv_branch: env j of this world becomes a copy of env j // s of ``src`` (this world has s x its envs)."""
        check(self.lib.rv_branch(self.h, src.h, int(s)))

    def plan_simulate(self, src, actions):
        """rv_plan_simulate with this world as the plan world: ``actions`` [N, S, H, G, 4] (N = src.n; [N, S, H, 4] when
        G = 1) are S action sequences of H steps per env of ``src``, which is only read.  Returns (states float32
        [N, S, H, RV_MAXB, 2] -- what ``plan_score`` takes --, rewards float32 [N, S, H], dones uint8 [N, S, H])."""
        a = self.torch.as_tensor(actions, dtype=self.torch.float32, device=self.device)
        if a.dim() == 4 and self.G == 1:
            a = a[:, :, :, None]
        if a.dim() != 5 or int(a.shape[0]) != src.n or tuple(a.shape[3:]) != (self.G, 4) or a.shape[1] < 1 or a.shape[2] < 1:
            raise ValueError('plan_simulate: actions must be [N, S, H, %d, 4] with N = %d, got %s' % (self.G, src.n, tuple(a.shape)))
        n, s, h = int(a.shape[0]), int(a.shape[1]), int(a.shape[2])
        a = a.contiguous()
        st = self._new((n, s, h, abi.RV_MAXB, 2), self.torch.float32)
        r = self._new((n, s, h), self.torch.float32)
        d = self._new((n, s, h), self.torch.uint8)
        check(self.lib.rv_plan_simulate(self.h, src.h, self._ptr(a), s, h, self._ptr(st), self._ptr(r), self._ptr(d)))
        return st, r, d

    # -- aimed pushes as proposals for look-ahead (include/rovat.h: rv_policy_heuristic_multi / rv_plan_propose)
    def _multi(self, fn, params, s):
        """``fn`` = rv_policy_heuristic_multi or rv_policy_route_multi: (actions float32 [M, s, G, 4], status int32 [M, s])"""
        s = int(s)
        rows = min(max(s, 1), abi.RV_HP_MAX_SAMPLES)      # (the library refuses an s outside [1, RV_HP_MAX_SAMPLES])
        a = self._new((self.n, rows, self.G, 4), self.torch.float32)
        st = self._new((self.n, rows), self.torch.int32)
        check(fn(self.h, C.byref(params), s, self._ptr(a), self._ptr(st)))
        return a, st

    def _propose(self, fn, src, params, s, h):
        """``fn`` = rv_plan_propose or rv_plan_propose_route, this world the plan world: (actions, states, rewards, dones,
        status)"""
        s, h = int(s), int(h)
        n, rs, rh = src.n, max(s, 1), max(h, 1)      # (the library refuses s < 1 and h < 1)
        a = self._new((n, rs, rh, self.G, 4), self.torch.float32)
        st = self._new((n, rs, rh, abi.RV_MAXB, 2), self.torch.float32)
        r = self._new((n, rs, rh), self.torch.float32)
        d = self._new((n, rs, rh), self.torch.uint8)
        status = self._new((n, rs, rh), self.torch.int32)
        check(fn(self.h, src.h, C.byref(params), s, h, self._ptr(a), self._ptr(st), self._ptr(r), self._ptr(d), self._ptr(status)))
        return a, st, r, d, status

    def policy_heuristic_multi(self, params, s):
        """rv_policy_heuristic_multi: ``s`` aimed pushes for every env of this world.  ``params``:
        ``push_proposal_params(...)``.  Returns (actions float32 [M, s, G, 4], status int32 [M, s]: abi.RV_HP_FOUND /
        abi.RV_HP_EXHAUSTED)."""
        return self._multi(self.lib.rv_policy_heuristic_multi, params, s)

    def plan_propose(self, src, params, s, h):
        """rv_plan_propose with this world as the plan world: ``s`` plans of ``h`` aimed pushes per env of ``src``, each
        push drawn from its branch's own simulated state; ``src`` is only read.  ``params``: ``push_proposal_params(...)``
        in 'spread' mode.  Returns (actions float32 [N, s, h, G, 4], states float32 [N, s, h, RV_MAXB, 2], rewards float32
        [N, s, h], dones uint8 [N, s, h] -- as ``plan_simulate`` -- and status int32 [N, s, h])."""
        return self._propose(self.lib.rv_plan_propose, src, params, s, h)

    # -- route-following pushes as proposals (include/rovat.h: rv_get_route_field / rv_policy_route_multi / rv_plan_propose_route)
    def route_field(self):
        """rv_get_route_field: uint8 [8, 8], the hops from every cell of the layout's grid through walkable cells to the
        nearest goal cell; abi.RV_PR_NONE where a cell is not walkable or reaches no goal."""
        d = self._new((abi.RV_PR_GRID, abi.RV_PR_GRID), self.torch.uint8)
        check(self.lib.rv_get_route_field(self.h, self._ptr(d)))
        return d

    def policy_route_multi(self, params, s):
        """rv_policy_route_multi: ``s`` pushes of body 0 along the layout for every env of this world.  ``params``:
        ``push_route_params(...)``.  Returns (actions float32 [M, s, G, 4], status int32 [M, s]: abi.RV_HP_FOUND /
        abi.RV_HP_EXHAUSTED)."""
        return self._multi(self.lib.rv_policy_route_multi, params, s)

    def plan_propose_route(self, src, params, s, h):
        """rv_plan_propose_route with this world as the plan world: ``plan_propose`` with the pushes of
        ``policy_route_multi``.  ``params``: ``push_route_params(...)``.  Returns (actions, states, rewards, dones, status)
        as ``plan_propose``."""
        return self._propose(self.lib.rv_plan_propose_route, src, params, s, h)

    # -- state
    def _get(self, fn, shape, dtype):
        t = self._new(shape, dtype)
        check(getattr(self.lib, fn)(self.h, self._ptr(t)))
        return t

    def body_state(self):
        return self._get('rv_get_body_state', (self.n, abi.RV_MAXB, 13), self.torch.float32)

    def set_body_state(self, s):
        check(self.lib.rv_set_body_state(self.h, self._ptr(self._in(s, (self.n, abi.RV_MAXB, 13), self.torch.float32))))

    def body_params(self):
        return self._get('rv_get_body_params', (self.n, abi.RV_MAXB, 8), self.torch.float32)

    def set_body_params(self, p):
        check(self.lib.rv_set_body_params(self.h, self._ptr(self._in(p, (self.n, abi.RV_MAXB, 8), self.torch.float32))))

    def joint_state(self):
        return self._get('rv_get_joint_state', (self.n, abi.RV_NJ, 2), self.torch.float32)

    def set_joint_state(self, s):
        check(self.lib.rv_set_joint_state(self.h, self._ptr(self._in(s, (self.n, abi.RV_NJ, 2), self.torch.float32))))

    def link_poses(self):
        return self._get('rv_get_link_poses', (self.n, abi.RV_NFRAME, 7), self.torch.float32)

    def env_counters(self):
        return self._get('rv_get_env_counters', (self.n, abi.RV_NCOUNTERS), self.torch.int32)

    def set_joint_targets(self, q, timeout=0.0, threshold=0.0):
        """timeout / threshold <= 0: the robot config's LIMB_TIMEOUT / LIMB_POSITION_THRESHOLD."""
        check(self.lib.rv_set_joint_targets(self.h, self._ptr(self._in(q, (self.n, abi.RV_NLIMB), self.torch.float32)),
                                            float(timeout), float(threshold)))

    def set_link_target(self, pose, timeout=0.0, threshold=0.0):
        check(self.lib.rv_set_link_target(self.h, self._ptr(self._in(pose, (self.n, 7), self.torch.float32)),
                                          float(timeout), float(threshold)))

    def set_link_path(self, poses, timeout=0.0, threshold=0.0):
        """poses [N, n_poses, 7] (or [n_poses, 7]: the same path for every env): SawyerSim.move_along_gripper_path
        -> ControllableBody.set_target_link_poses."""
        p = self.torch.as_tensor(poses, dtype=self.torch.float32, device=self.device)
        if p.dim() == 2:
            p = p[None].expand(self.n, -1, -1)
        n_poses = int(p.shape[1])
        p = p.reshape(self.n, n_poses, 7).contiguous()
        check(self.lib.rv_set_link_path(self.h, self._ptr(p), n_poses, float(timeout), float(threshold)))

    def set_max_joint_velocities(self, vmax):
        """rv_set_max_joint_velocities: speed limits [N, 7] (or [7]) of the limb joints for the targets being followed."""
        v = self._in(np.broadcast_to(np.asarray(vmax, np.float32), (self.n, abi.RV_NLIMB)).copy(), (self.n, abi.RV_NLIMB), self.torch.float32)
        check(self.lib.rv_set_max_joint_velocities(self.h, self._ptr(v)))

    def robot_ready(self):
        """[N, 2] uint8: (is_limb_ready, is_gripper_ready) -- retires finished targets like the reference's query."""
        return self._get('rv_get_robot_ready', (self.n, 2), self.torch.uint8)

    def reset_targets(self):
        check(self.lib.rv_reset_targets(self.h))

    def set_motor_targets(self, q, mask=None):
        """position_control_array: POSITION_CONTROL targets for the masked joints."""
        qt = self._in(q, (self.n, abi.RV_NJ), self.torch.float32)
        mt = None if mask is None else self._in(mask, (self.n, abi.RV_NJ), self.torch.uint8)
        check(self.lib.rv_set_motor_targets(self.h, self._ptr(qt), None if mt is None else self._ptr(mt)))

    def grip(self, value):
        check(self.lib.rv_grip(self.h, float(value)))

    JOINT_TYPES = {'revolute': 0, 'prismatic': 1, 'fixed': 4, 'point2point': 5}      # pybullet.JOINT_REVOLUTE / _PRISMATIC / _FIXED / _POINT2POINT: the reference's JOINT_TYPES_MAPPING

    def set_constraint(self, body, target7, frame7=None, max_force=500.0, child=-1, joint_type='fixed'):
        """rv_set_constraint_ex: tie frame7 (in the body frame; None = the body frame) of movable body ``body`` to
        the frame target7 -- of the world (child = -1) or, given in its frame, of movable body ``child`` or of frame f of the arm
        (child = abi.RV_CHILD_LINK(f): fixed / point2point only) -- by a
        'fixed', a 'point2point' or a 'prismatic' joint (sliding along the x axis of the target frame) with at most
        max_force N per row; max_force < 0 removes it."""
        if joint_type not in self.JOINT_TYPES:
            raise NotImplementedError("joint types built: 'fixed', 'point2point', 'prismatic', 'revolute' (not %r)" % (joint_type,))
        t = (C.c_float * 7)(*[float(x) for x in (target7 if target7 is not None else [0, 0, 0, 0, 0, 0, 1])])
        f = None if frame7 is None else (C.c_float * 7)(*[float(x) for x in frame7])
        check(self.lib.rv_set_constraint_ex(self.h, int(body), int(child), self.JOINT_TYPES[joint_type], f, t, float(max_force)))

    def remove_constraint(self, body):
        check(self.lib.rv_set_constraint(self.h, int(body), None, None, -1.0))

    def set_friction(self, mu_finger=-1.0, mu_table=-1.0):
        """rv_set_friction: lateral friction of the finger-tip pads / the table top (negative: unchanged)."""
        check(self.lib.rv_set_friction(self.h, float(mu_finger), float(mu_table)))

    def set_gravity(self, gravity):
        g = (C.c_float * 3)(float(gravity[0]), float(gravity[1]), float(gravity[2]))
        check(self.lib.rv_set_gravity(self.h, g))

    def state_view(self):
        """Zero-copy READ-ONLY torch views of the resident env blocks (rv_get_state_ptrs)."""
        v = abi.rv_state_view()
        check(self.lib.rv_get_state_ptrs(self.h, C.byref(v)))
        words = int(v.env_stride_bytes) // 4

        class _Raw(object):
            pass
        raw = _Raw()
        raw.__cuda_array_interface__ = {'shape': (self.n, words), 'typestr': '<f4', 'data': (int(v.d_envs), False),
                                        'version': 2, 'strides': None}
        t = self.torch
        blocks = t.as_tensor(raw, device=self.device)

        def f(off, count, shape):
            return blocks[:, int(off) // 4: int(off) // 4 + count].reshape((self.n,) + shape)
        return {
            'body': f(v.off_body, abi.RV_MAXB * 13, (abi.RV_MAXB, 13)),
            'active': f(v.off_active, abi.RV_MAXB, (abi.RV_MAXB,)).view(t.int32),
            'joint_q': f(v.off_joint_q, abi.RV_NJ, (abi.RV_NJ,)),
            'joint_qd': f(v.off_joint_qd, abi.RV_NJ, (abi.RV_NJ,)),
            'link_pos': f(v.off_link_pos, abi.RV_NFRAME * 3, (abi.RV_NFRAME, 3)),
            'link_quat': f(v.off_link_quat, abi.RV_NFRAME * 4, (abi.RV_NFRAME, 4)),
            'obs_pos': f(v.off_obs_pos, abi.RV_MAXB * 3, (abi.RV_MAXB, 3)),
            'table_z': f(v.off_table_z, 1, ()),
        }

    def compute_ik(self, pose):
        p = self._in(pose, (self.n, 7), self.torch.float32)
        q = self._new((self.n, abi.RV_NLIMB), self.torch.float32)
        check(self.lib.rv_compute_ik(self.h, self._ptr(p), self._ptr(q)))
        return q

    def camera(self):
        """[N, 17] float32: fx, fy, cx, cy, skew, rotation (row-major), translation -- the calibration each env is observed
        with (rv_config's plus the noise of its last reset, KINECT2.DEPTH.*_NOISE)."""
        return self._get('rv_get_camera', (self.n, 17), self.torch.float32)

    def query_contacts(self):
        return self._get('rv_query_contacts', (self.n, 2 + abi.RV_MAXB), self.torch.uint8)

    def manifold_counts(self):
        return self._get('rv_get_manifold_counts', (self.n, abi.RV_NMAN), self.torch.int32)

    def contact_points(self, body_a=-1, link_a=-1, body_b=-1, link_b=-1, capacity=abi.RV_CP_MAX):
        """rv_get_contact_points: PyBullet's contact records (getContactPoints) of every env, filtered by the query
        (-1 = any; bodies are slots 0..RV_MAXB-1, RV_CP_TABLE, RV_CP_ARM; links only for the arm) and oriented so
        that body_a is body A.  Returns device tensors, with no host sync: ids int32 [N, capacity, 4] (bodyA, bodyB,
        linkA, linkB), data float32 [N, capacity, RV_CP_NF] (positionOnA, positionOnB, contactNormalOnB,
        contactDistance, normalForce, lateralFriction1, lateralFrictionDir1, lateralFriction2, lateralFrictionDir2)
        and count int32 [N] -- the number of matches; only the first min(count, capacity) rows are written."""
        q = abi.rv_contact_query(int(body_a), int(link_a), int(body_b), int(link_b))
        cap = int(capacity)
        ids = self._new((self.n, max(cap, 1), 4), self.torch.int32)
        data = self._new((self.n, max(cap, 1), abi.RV_CP_NF), self.torch.float32)
        count = self._new((self.n,), self.torch.int32)
        check(self.lib.rv_get_contact_points(self.h, C.byref(q), cap, self._ptr(ids), self._ptr(data), self._ptr(count)))
        return ids, data, count

    def contact_forces(self, body_a=-1, link_a=-1, body_b=-1, link_b=-1):
        """The net contact force on body A, [N, 3] float32 on the device: fn n + f1 d1 + f2 d2 summed over the records
        of contact_points(...) (n points from B to A)."""
        ids, data, count = self.contact_points(body_a, link_a, body_b, link_b)
        valid = self.torch.arange(data.shape[1], device=self.device)[None, :] < count[:, None]
        f = (data[..., 10:11] * data[..., 6:9] + data[..., 11:12] * data[..., 12:15] + data[..., 15:16] * data[..., 16:19])
        return self.torch.where(valid[..., None], f, self.torch.zeros_like(f)).sum(dim=1)

    def observe(self, point_cloud=False, pose_modes=False):
        out, b = self._obs_buffers((self.n,), point_cloud, pose_modes)
        check(self.lib.rv_observe(self.h, C.byref(b)))
        return out

    def render(self, segmask=True):
        """Depth image [N, H, W] (eye z, 0 = nothing hit) and segmentation mask of the simulated camera."""
        h, w = int(self.cfg.cam_height), int(self.cfg.cam_width)
        depth = self._new((self.n, h, w), self.torch.float32)
        seg = self._new((self.n, h, w), self.torch.uint8) if segmask else None
        check(self.lib.rv_render(self.h, self._ptr(depth), self._ptr(seg) if segmask else None))
        return depth, seg

    def render_rgb(self):
        """rv_render_rgb: uint8 [N, H, W, 3]."""
        rgb = self._new((self.n, int(self.cfg.cam_height), int(self.cfg.cam_width), 3), self.torch.uint8)
        check(self.lib.rv_render_rgb(self.h, self._ptr(rgb)))
        return rgb

    def view_inputs(self, cameras, env_index=None, height=None, width=None):
        """What ``render_view`` makes of its first four arguments: (rows float32 [V, 17], env index int32 [V], height,
        width), NumPy arrays on the host."""
        from robovat_amd.perception.camera import Camera, camera_row
        torch = self.torch
        h0, w0 = int(self.cfg.cam_height), int(self.cfg.cam_width)
        if isinstance(cameras, Camera):
            cameras = [cameras]
        if isinstance(cameras, (list, tuple)) and len(cameras) and all(isinstance(c, Camera) for c in cameras):
            if cameras[0].height is not None and cameras[0].width is not None:
                h0, w0 = int(cameras[0].height), int(cameras[0].width)
            rows = np.stack([camera_row(c) for c in cameras])
        else:
            if torch.is_tensor(cameras):
                cameras = cameras.detach().cpu().numpy()
            rows = np.asarray(cameras, dtype=np.float32)
            if rows.ndim == 1:
                rows = rows[None]
        if rows.ndim != 2 or rows.shape[1] != 17 or rows.shape[0] < 1:
            raise ValueError('render_view: cameras must be a Camera, a sequence of them or rows [V, 17], got %s' % (tuple(rows.shape),))
        if env_index is None:
            idx = np.arange(self.n, dtype=np.int32) if rows.shape[0] in (1, self.n) else None
            if idx is None:
                raise ValueError('render_view: %d cameras need an env_index (the world has %d envs)' % (rows.shape[0], self.n))
        else:
            if torch.is_tensor(env_index):
                env_index = env_index.detach().cpu().numpy()
            idx = np.asarray(env_index)
            if idx.dtype.kind not in 'iu':
                raise ValueError('render_view: env_index must be integers')
            idx = idx.reshape(-1).astype(np.int64)
            if idx.size and (idx.min() < -2 ** 31 or idx.max() >= 2 ** 31):
                raise ValueError('render_view: env index outside [0, N)')
            idx = idx.astype(np.int32)
        v = max(int(rows.shape[0]), int(idx.size))
        if rows.shape[0] == 1:
            rows = np.repeat(rows, v, axis=0)
        if idx.size == 1:
            idx = np.repeat(idx, v)
        if rows.shape[0] != v or idx.size != v:
            raise ValueError('render_view: %d cameras and %d env indices' % (rows.shape[0], idx.size))
        rows, idx = np.ascontiguousarray(rows, dtype=np.float32), np.ascontiguousarray(idx, dtype=np.int32)
        h, w = int(h0 if height is None else height), int(w0 if width is None else width)
        return rows, idx, h, w

    def render_view(self, cameras, env_index=None, height=None, width=None, supersample=1, rgb=True, depth=False,
                    segmask=False, out=None):
        """rv_render_view: free camera views of chosen envs.  ``cameras``: a ``perception.Camera`` (``perception.look_at``),
        a sequence of them, or calibration rows [V, 17] / [17] as ``camera()`` returns them; ``env_index``: the env each
        view looks at (None: all N envs, in order).  One camera is broadcast over ``env_index``, one env over the cameras.
        ``height`` / ``width`` default to the first camera's own (rows: the config's).  ``supersample`` = s: s x s rays per
        rgb pixel, box-filtered (rgb only).  ``out``: None, or a dict with contiguous tensors of this device to write --
        'rgb' uint8 [V, H, W, 3], 'depth' float32 [V, H, W], 'segmask' uint8 [V, H, W]; a key in ``out`` asks for that image
        whatever the flags say.  Returns a dict of the images asked for, device tensors; nothing is synchronised."""
        torch = self.torch
        rows, idx, h, w = self.view_inputs(cameras, env_index, height, width)
        v = int(rows.shape[0])
        p = view_params(v, h, w, supersample)
        want = {'rgb': (bool(rgb), torch.uint8, (v, h, w, 3)), 'depth': (bool(depth), torch.float32, (v, h, w)),
                'segmask': (bool(segmask), torch.uint8, (v, h, w))}
        out = dict(out or {})
        unknown = set(out) - set(want)
        if unknown:
            raise ValueError('render_view: out has unknown keys %s' % (sorted(unknown),))
        res = {}
        for key, (flag, dtype, shape) in want.items():
            t = out.get(key)
            if t is not None:
                if not (torch.is_tensor(t) and t.dtype == dtype and t.device == self.device and tuple(t.shape) == shape
                        and t.is_contiguous()):
                    raise ValueError('render_view: out[%r] must be a contiguous %s %s tensor on %s' % (key, dtype, shape, self.device))
                res[key] = t
            elif flag:
                res[key] = self._new(shape, dtype)
        opt = lambda key: self._ptr(res[key]) if key in res else None
        check(self.lib.rv_render_view(self.h, C.byref(p), idx.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p),
                                      opt('rgb'), opt('depth'), opt('segmask')))
        return res

    def reward(self):
        r = self._new((self.n,), self.torch.float32)
        d = self._new((self.n,), self.torch.uint8)
        check(self.lib.rv_reward(self.h, self._ptr(r), self._ptr(d)))
        return r, d

    def episode_returns(self):
        return self._get('rv_get_episode_returns', (self.n,), self.torch.float32)

    def stats(self):
        s = abi.rv_macro_stats()
        check(self.lib.rv_get_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}

    def last_kernel_ms(self):
        ms = C.c_float()
        check(self.lib.rv_last_kernel_ms(self.h, C.byref(ms)))
        return float(ms.value)
