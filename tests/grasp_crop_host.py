"""rv_grasp_crops restated in float32 NumPy, operation for operation (csrc/rv_dev_grasp_sampler.h), the
float64 composition of the host mirrors it stands for, and the grasp rows the CPU and GPU tests share.

``crops(depth, grasps, h, w, step)`` is the kernel: every product and every sum is a float32 operation of its own, in
the kernel's order.  ``composition(depth_n, row, h, w, step)`` is ``crop(transform(...))[step//2::step, step//2::step]``
with ``depth_utils`` in float64, and ``source_coords`` gives the float64 source coordinates of every output pixel, which
is how a test tells a pixel at a rounding boundary from the rest."""
import numpy as np

from robovat_amd.perception import depth_utils

f32 = np.float32


def frame(rows, H, W, h, w, step):
    """c, s, gx, gy [R] and x0, y0 (scalars) of the kernel's gc_frame, float32"""
    g = np.asarray(rows, f32).reshape(-1, 5)
    x1, y1, x2, y2 = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    with np.errstate(all='ignore'):
        ax, ay = x2 - x1, y2 - y1
        ln = np.sqrt(ax * ax + ay * ay)
        ok = (ln > f32(0.0)) & (ln <= f32(3.402823466e38))
        safe = np.where(ok, ln, f32(1.0))
        c = np.where(ok, ax / safe, f32(1.0)).astype(f32)
        s = np.where(ok, ay / safe, f32(0.0)).astype(f32)
        gx, gy = f32(0.5) * (x1 + x2), f32(0.5) * (y1 + y2)
    hw, hh = f32(0.5) * f32(W), f32(0.5) * f32(H)
    x0 = np.floor(hw - f32(0.5) * f32(w * step)) - hw
    y0 = np.floor(hh - f32(0.5) * f32(h * step)) - hh
    return c, s, gx.astype(f32), gy.astype(f32), f32(x0), f32(y0)


def crops(depth, grasps, h, w, step):
    """depth [N, H, W] float32, grasps [N, K, 5] -> (images [N, K, h, w] float32, grasp depths [N, K] float32)"""
    depth = np.asarray(depth, f32)
    g = np.asarray(grasps, f32)
    N, H, W = depth.shape
    K = g.shape[1]
    c, s, gx, gy, x0, y0 = frame(g, H, W, h, w, step)
    c, s, gx, gy = (v.reshape(N, K, 1, 1) for v in (c, s, gx, gy))
    ox = (x0 + (np.arange(w) * step + step // 2).astype(f32)).astype(f32).reshape(1, 1, 1, w)
    oy = (y0 + (np.arange(h) * step + step // 2).astype(f32)).astype(f32).reshape(1, 1, h, 1)
    with np.errstate(all='ignore'):
        sx = ((c * ox - s * oy).astype(f32) + gx).astype(f32)
        sy = ((s * ox + c * oy).astype(f32) + gy).astype(f32)
        inside = (sx >= f32(-0.5)) & (sx < f32(W) - f32(0.5)) & (sy >= f32(-0.5)) & (sy < f32(H) - f32(0.5))
        fx = np.floor((sx + f32(0.5)).astype(f32))
        fy = np.floor((sy + f32(0.5)).astype(f32))
    ix = np.minimum(np.where(inside, fx, 0).astype(np.int64), W - 1)
    iy = np.minimum(np.where(inside, fy, 0).astype(np.int64), H - 1)
    n = np.arange(N).reshape(N, 1, 1, 1)
    out = np.where(inside, depth[n, iy, ix], f32(0.0)).astype(f32)
    return out, g[:, :, 4].copy()


def angle_and_centre(row):
    """theta of p2 - p1 and the midpoint in float64, with the kernel's rule for a degenerate axis (theta 0)"""
    x1, y1, x2, y2 = (float(v) for v in np.asarray(row, np.float64)[:4])
    ln = np.hypot(x2 - x1, y2 - y1)
    theta = np.arctan2(y2 - y1, x2 - x1) if ln > 0 and np.isfinite(ln) else 0.0
    return theta, 0.5 * (x1 + x2), 0.5 * (y1 + y2)


def composition(image, row, h, w, step):
    """crop(transform(image, (H/2 - g_y, W/2 - g_x), theta), h*step, w*step)[step//2::step, step//2::step], float64 maps"""
    H, W = image.shape
    theta, gx, gy = angle_and_centre(row)
    t = depth_utils.transform(image, (H / 2.0 - gy, W / 2.0 - gx), theta)
    return depth_utils.crop(t, h * step, w * step)[step // 2::step, step // 2::step]


def source_coords(row, H, W, h, w, step):
    """float64 source coordinates (sx, sy), each [h, w], of the output pixels of one row: the inverse map of
    ``depth_utils.transform`` at the window positions of ``depth_utils.crop``"""
    theta, gx, gy = angle_and_centre(row)
    c, s = np.cos(theta), np.sin(theta)
    x = np.floor(W / 2.0 - (w * step) / 2.0) + np.arange(w) * step + step // 2
    y = np.floor(H / 2.0 - (h * step) / 2.0) + np.arange(h) * step + step // 2
    ox, oy = np.meshgrid(x - W / 2.0, y - H / 2.0)
    return gx + (c * ox - s * oy), gy + (s * ox + c * oy)


def ramp(N, H, W):
    """depth[n, y, x] = 1 + (n*H + y)*W + x: every value is unique and exact in float32, so any wrong index shows"""
    return (1 + np.arange(N * H * W, dtype=np.int64)).astype(f32).reshape(N, H, W)


def tie_rows(H, W):
    """[R, 5] rows whose source coordinates sit on rounding boundaries: horizontal and vertical grasps with integer
    endpoints and half-integer centres (every source coordinate an exact .5), p1 == p2, and a 45 degree grasp"""
    cx, cy = W // 2, H // 2
    return np.array([
        [cx - 3, cy, cx + 4, cy, 0.51],          # horizontal, gx = cx + .5
        [cx + 4, cy, cx - 3, cy, 0.52],            # horizontal, pointing left
        [cx, cy - 2, cx, cy + 3, 0.53],            # vertical, gy = cy + .5
        [cx, cy + 3, cx, cy - 2, 0.54],            # vertical, pointing up
        [cx - 2, cy - 3, cx + 3, cy - 3, 0.55],    # horizontal, off centre
        [cx, cy, cx, cy, 0.56],                    # p1 == p2
        [cx + 0.5, cy - 0.5, cx + 0.5, cy - 0.5, 0.57],      # p1 == p2 at a half-integer point
        [cx - 3, cy - 3, cx + 3, cy + 3, 0.58],    # 45 degrees
    ], f32)


def generic_rows(count, H, W, seed):
    """[count, 5] seeded rows: endpoints uniform over the image plus 5 px, length 2 to 60 px"""
    rng = np.random.RandomState(seed)
    rows = np.zeros((count, 5), f32)
    for r in range(count):
        while True:
            p = rng.uniform([-5.0, -5.0], [W + 5.0, H + 5.0])
            ln, th = rng.uniform(2.0, 60.0), rng.uniform(-np.pi, np.pi)
            q = p + ln * np.array([np.cos(th), np.sin(th)])
            if -5.0 <= q[0] <= W + 5.0 and -5.0 <= q[1] <= H + 5.0:
                break
        rows[r] = [p[0], p[1], q[0], q[1], rng.uniform(0.3, 1.0)]
    return rows


def edge_rows(H, W):
    """([R, 5] rows, all_zero [R]): NaN, +-inf and 1e30 coordinates and centres far outside give all-zero images; centres
    40 px outside each corner (all zero or partly zero by the window's size: all_zero None = the spec decides)"""
    nan, inf = np.nan, np.inf
    rows = [
        ([nan, 3, 8, 3, 0.61], True), ([2, nan, 8, 3, 0.62], True), ([2, 3, nan, nan, 0.63], True),
        ([inf, 3, 8, 3, 0.64], True), ([2, -inf, 8, 3, 0.65], True), ([inf, inf, inf, inf, 0.66], True),
        ([-inf, 3, inf, 3, 0.67], True), ([1e30, 3, 8, 3, 0.68], True), ([2, 3, 8, -1e30, 0.69], True),
        ([1e30, 1e30, 1e30, 1e30, 0.70], True), ([3e38, 3, 2e38, 3, 0.71], True),
        ([-44, -40, -36, -40, 0.72], None), ([W + 36, -40, W + 44, -40, 0.73], None),
        ([-44, H + 40, -36, H + 40, 0.74], None), ([W + 36, H + 40, W + 44, H + 40, 0.75], None),
        ([-40, -44, -40, -36, 0.76], None),
        ([-3, -2, 3, 2, 0.77], False), ([W - 3, H - 2, W + 3, H + 2, 0.78], False),      # a corner inside the window
    ]
    return np.array([r for r, _ in rows], f32), [z for _, z in rows]
