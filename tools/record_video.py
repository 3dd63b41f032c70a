#!/usr/bin/env python
"""Watch a few steps of an env: one file per recorded env and episode, and one contact sheet of every n-th frame.

    python tools/record_video.py --env VecPushEnv --policy HeuristicPushPolicy --num_steps 4 --output_dir recordings
    python tools/record_video.py --env VecPushEnv --task crossing --layout_id 1 --policy CEMPushPolicy --plan 16 2 --envs 0 3 --eye 1.5 -0.9 0.7
    python tools/record_video.py --env VecGrasp4DofEnv --policy AntipodalGrasp4DofPolicy --num_steps 2 --format gif

The env is built with the ``RECORDING`` option (``robovat_amd/envs/recording.py``): a camera at ``--eye`` looking at
``--target`` (defaults: a corner view of the point 5 cm above the table centre), a frame every ``--every`` substeps, played
at ``--fps``.  Formats: png (animated, lossless), gif, npz -- no video codec is a dependency.  The contact sheet
``<output_dir>/sheet_env<row>.png`` shows every ``--sheet_every``-th frame of the first episode of each recorded env.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--env', default='VecPushEnv', choices=['VecPushEnv', 'VecGrasp4DofEnv'])
    ap.add_argument('--policy', default='RandomPolicy')
    ap.add_argument('--plan', type=int, nargs=2, default=[16, 2], metavar=('SAMPLES', 'HORIZON'),
                    help='candidates and steps per decision of the look-ahead push policies (ShootingPushPolicy, '
                         'HeuristicShootingPushPolicy, RouteShootingPushPolicy, CEMPushPolicy)')
    ap.add_argument('--num_envs', type=int, default=4)
    ap.add_argument('--num_steps', type=int, default=4, help='steps in all; an env whose episode ends is reset')
    ap.add_argument('--envs', type=int, nargs='+', default=[0], help='the env rows that are recorded')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--task', default=None)
    ap.add_argument('--layout_id', type=int, default=0)
    ap.add_argument('--max_steps', type=int, default=4)
    ap.add_argument('--eye', type=float, nargs=3, default=None)
    ap.add_argument('--target', type=float, nargs=3, default=None)
    ap.add_argument('--height', type=int, default=240)
    ap.add_argument('--width', type=int, default=320)
    ap.add_argument('--fov_y_deg', type=float, default=45.0)
    ap.add_argument('--supersample', type=int, default=2)
    ap.add_argument('--every', type=int, default=50, help='substeps between two frames')
    ap.add_argument('--fps', type=float, default=20.0)
    ap.add_argument('--format', default='png', choices=['png', 'gif', 'npz'])
    ap.add_argument('--sheet_every', type=int, default=8)
    ap.add_argument('--output_dir', default='recordings')
    args = ap.parse_args()
    import numpy as np
    from robovat_amd import configs, envs, policies
    from robovat_amd.io.video_utils import contact_sheet, read_frames
    from robovat_amd.perception import look_at
    np.random.seed(args.seed)
    grasp = args.env == 'VecGrasp4DofEnv'
    base = configs.grasp_env_config() if grasp else configs.push_env_config(TASK_NAME=args.task, LAYOUT_ID=args.layout_id, MAX_STEPS=args.max_steps)
    table = base.SIM.TABLE.POSE[0]
    centre = np.array([table[0], table[1], table[2]], dtype=np.float64)
    eye = np.array(args.eye) if args.eye else centre + np.array([0.9, -0.9, 0.7])
    target = np.array(args.target) if args.target else centre + np.array([0.0, 0.0, 0.05])
    cam = look_at(eye, target, height=args.height, width=args.width, fov_y_deg=args.fov_y_deg)
    base['RECORDING'] = configs.AttrDict({
        'USE': True, 'NUM_STEPS': args.every, 'FPS': args.fps, 'OUTPUT_DIR': args.output_dir, 'ENVS': args.envs,
        'SUPERSAMPLE': args.supersample, 'FORMAT': args.format,
        'CAMERA': {'HEIGHT': args.height, 'WIDTH': args.width, 'INTRINSICS': np.asarray(cam.intrinsics).tolist(),
                   'TRANSLATION': np.asarray(cam.translation).tolist(), 'ROTATION': np.asarray(cam.rotation).tolist()}})
    env = (envs.VecGrasp4DofEnv if grasp else envs.VecPushEnv)(args.num_envs, config=base, seed=args.seed)
    cls = getattr(policies, args.policy)
    policy = cls(env, args.plan[0], args.plan[1]) if args.policy.endswith('PushPolicy') and args.policy != 'HeuristicPushPolicy' else cls(env)
    obs = env.reset()
    for k in range(args.num_steps):
        obs, reward, done, _ = env.step(policy.action(obs))
        print('step %d: mean reward %.3f, %d of %d episodes over' % (k, float(reward.float().mean()), int(done.sum()), args.num_envs))
        if bool(done.any()) and k + 1 < args.num_steps:
            obs = env.reset(done)
    env.close()
    paths = env._recorder.paths
    for p in paths:
        print('wrote %s (%d bytes)' % (p, os.path.getsize(p)))
    for row in args.envs:
        first = [p for p in paths if os.path.basename(p).startswith('env%d_ep0000' % row)]
        if first:
            frames, _ = read_frames(first[0])
            sheet = os.path.join(args.output_dir, 'sheet_env%d.png' % row)
            shown = contact_sheet(frames, sheet, every=args.sheet_every)
            print('wrote %s: frames %s of %d' % (sheet, shown, len(frames)))


if __name__ == '__main__':
    main()
