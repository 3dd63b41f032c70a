"""Push-task reward functions, host (numpy) edition.

Same call signature as ``robovat/reward_fns/push_reward.py:272-405``:
``get_reward_fn(task_name, layout_id, ...)(state, next_state) -> (reward,
termination)`` on ``[batch, bodies, 2]`` arrays (or observation dicts).  The
device computes the identical quantity inside ``rv_step_macro``; this module is
for API users and for the golden-vector tests.  The behaviour pinned by the
goldens includes the reference's quirks that downstream users see
(SURVEY.md Appendix B-8): the clearing score's overwritten minimum, the
all-False insertion termination outside planning mode, and tile centres that
move with the ``size`` argument of ``check_on_tiles``.

``is_planning=True`` is the transition check a sampling-based planner scores
candidate plans with (``push_reward.py:110-151, 168-200, 230-269, 312-357``):
stride limits, table border, target border and the two middle states of the
straight line between the states; its termination penalty is not masked by
the goal.  ``rv_plan_reward`` / ``rv_plan_score`` compute it on the device.
"""
import numpy as np

from robovat_amd.envs.push import push_layouts

CLEARING_GOAL_X = 0.7
CLEARING_GOAL_Y = 0.9


def process_state(state):
    if isinstance(state, dict):
        if 'position' in state:
            state = np.asarray(state['position'])[..., :2]
        else:
            state = np.mean(np.asarray(state['point_cloud']), axis=-2)[..., :2]
        if state.ndim == 2:
            state = state[np.newaxis]
    state = np.asarray(state)
    assert state.shape[-1] == 2
    return state


def _tile_centres(centers, size, offset):
    return np.asarray(offset, dtype=np.float64) + np.asarray(centers, dtype=np.float64) * size


def check_on_tiles(position, centers, size, offset, max_dist=None):
    max_dist = size if max_dist is None else max_dist
    d = np.abs(position[:, None, :] - _tile_centres(centers, size, offset)[None])
    return np.any((d[..., 0] <= 0.5 * max_dist) & (d[..., 1] <= 0.5 * max_dist), axis=1)


def get_tile_dists(position, centers, size, offset):
    d = position[:, None, :] - _tile_centres(centers, size, offset)[None]
    return np.linalg.norm(d, axis=-1).min(axis=1)


def _score(task, state, layout):
    if task == 'clearing':
        d1 = np.mean(np.abs(state[:, :, 0] - CLEARING_GOAL_X), axis=1)
        d3 = np.mean(np.abs(state[:, :, 1] + CLEARING_GOAL_Y), axis=1)
        return -np.minimum(d1, d3)
    return -get_tile_dists(state[:, 0, :], layout.goal, layout.size, layout.offset)


def _goal(task, state, layout):
    if task == 'clearing':
        ok = np.ones(state.shape[0], dtype=bool)
        for i in range(state.shape[1]):
            ok &= ~check_on_tiles(state[:, i, :], layout.region, layout.size * 1.25, layout.offset)
        return ok
    return check_on_tiles(state[:, 0, :], layout.goal, layout.size, layout.offset)


def _termination(task, next_state, layout):
    if task == 'crossing':
        return ~check_on_tiles(next_state[:, 0, :], layout.region, layout.size, layout.offset,
                               max_dist=layout.size * 1.5)
    return np.zeros(next_state.shape[0], dtype=bool)


def _middle_states(state, next_state):
    return state + (1. / 3.) * (next_state - state), state + (2. / 3.) * (next_state - state)


def _planning_termination(task, state, next_state, layout):
    """insertion_termination / crossing_termination with is_planning=True (push_reward.py:110-151, 168-200)."""
    term = np.zeros(next_state.shape[0], dtype=bool)
    if task == 'insertion':
        size = layout.size * 1.25
        for s in (next_state,) + _middle_states(state, next_state):
            for i in range(next_state.shape[1]):
                term |= check_on_tiles(s[:, i, :], layout.region, size, layout.offset)
    elif task == 'crossing':
        on_bridge = np.ones(next_state.shape[0], dtype=bool)
        for s in (next_state,) + _middle_states(state, next_state):
            on_bridge &= check_on_tiles(s[:, 0, :], layout.region, layout.size, layout.offset, max_dist=layout.size)
        term = ~on_bridge
    return term


def check_stride(state, next_state, min_stride, max_stride):
    strides = np.linalg.norm(next_state - state, axis=-1)
    return np.all(strides < min_stride, axis=1) | np.any(strides > max_stride, axis=1)


def _outside(x, y, x_range, y_range, tolerance):
    return ((x < x_range[0] - tolerance) | (x > x_range[1] + tolerance) |
            (y < y_range[0] - tolerance) | (y > y_range[1] + tolerance))


def check_border(state, next_state, x_range=(0.22, 0.98), y_range=(-0.56, 0.66), tolerance=0.02):
    return np.any(_outside(next_state[..., 0], next_state[..., 1], x_range, y_range, tolerance), axis=1)


def check_target_border(state, next_state, x_range=(0.3, 0.8), y_range=(-0.56, 0.66), tolerance=0.02):
    return _outside(next_state[:, 0, 0], next_state[:, 0, 1], x_range, y_range, tolerance)


def dummy_reward_fn(state, next_state):
    state = process_state(state)
    shape = () if state.ndim == 2 else (state.shape[0],)
    return np.ones(shape, dtype=np.float32), np.zeros(shape, dtype=bool)


def get_reward_fn(task_name, layout_id, goal_reward=100.0, termination_reward=-100.0,
                  dense_reward=1.0, time_reward=-1.0, use_dense_reward=True,
                  use_time_penalty=True, is_planning=False, is_high_level=False):
    if task_name is None or task_name == 'data_collection':
        return dummy_reward_fn
    if task_name not in push_layouts.TASK_NAME_TO_LAYOUTS:
        raise ValueError('Unrecognized manipulation task: %r' % task_name)
    layout = push_layouts.TASK_NAME_TO_LAYOUTS[task_name][layout_id]

    def planning_reward_fn(state, next_state):
        state, next_state = process_state(state), process_state(next_state)
        if is_high_level:
            termination = check_stride(state, next_state, min_stride=0.1, max_stride=0.3)
        else:
            termination = check_stride(state, next_state, min_stride=0.01, max_stride=0.15)
        termination = termination | check_border(state, next_state)
        if task_name == 'insertion':
            termination = termination | check_target_border(state, next_state)
        termination = termination | _planning_termination(task_name, state, next_state, layout)
        goal = _goal(task_name, next_state, layout) & ~termination
        # (the float32 accumulator and the order of its updates are the reference's, :309-370; the penalty
        # is not masked by the goal in planning mode, :351-357)
        reward = np.zeros(state.shape[0], dtype=np.float32)
        reward += goal_reward * goal.astype(np.float32)
        reward += termination_reward * termination.astype(np.float32)
        if use_dense_reward:
            reward += np.abs(_score(task_name, next_state, layout) - _score(task_name, state, layout)) * dense_reward
        if use_time_penalty:
            reward += time_reward
        return reward, termination | goal

    if is_planning:
        return planning_reward_fn

    def reward_fn(state, next_state):
        state, next_state = process_state(state), process_state(next_state)
        termination = _termination(task_name, next_state, layout)
        goal = _goal(task_name, next_state, layout) & ~termination
        reward = np.zeros(state.shape[0], dtype=np.float32)
        reward += goal_reward * goal.astype(np.float32)
        reward += termination_reward * (termination & ~goal).astype(np.float32)
        if use_dense_reward:
            reward += (np.abs(_score(task_name, next_state, layout) - _score(task_name, state, layout))
                       * dense_reward).astype(np.float32)
        if use_time_penalty:
            reward += time_reward
        return reward, termination | goal

    return reward_fn


class PushReward(object):
    """Reward function object with the reference's interface (push_reward.py:377-405)."""

    def __init__(self, name, task_name, layout_id, is_planning=False):
        self.name = name
        self.env = None
        self.reward_fn = get_reward_fn(task_name=task_name, layout_id=layout_id, is_planning=is_planning)

    def initialize(self, env):
        self.env = env

    def on_episode_start(self):
        pass

    def on_episode_end(self):
        pass

    def get_reward(self):
        assert self.env.prev_obs_data is not None and self.env.obs_data is not None
        reward, termination = self.reward_fn(self.env.prev_obs_data, self.env.obs_data)
        return float(np.asarray(reward).reshape(-1)[0]), bool(np.asarray(termination).reshape(-1)[0])
