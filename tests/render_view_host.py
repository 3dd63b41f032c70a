"""Host-side restatements for the rv_render_view tests: the camera row of the supersampled image and the
integer box filter, as include/rovat.h words them, in NumPy -- and the free views of tests/test_gpu_render_view.py."""
import numpy as np

from robovat_amd.perception import look_at


def scaled_row(row, s):
    """The calibration row of the s-times larger image, in float32 with one rounding per operation: fx' = s fx, fy' = s fy,
    skew' = s skew, cx' = s cx + (s - 1) / 2, cy' = s cy + (s - 1) / 2; rotation and translation stay."""
    out = np.array(row, dtype=np.float32).copy()
    f, off = np.float32(s), np.float32(0.5 * (s - 1))      # ((s - 1) / 2 is exact in float32 for every s)
    for k in (0, 1, 4):
        out[..., k] = f * out[..., k]
    for k in (2, 3):
        out[..., k] = f * out[..., k] + off
    return out


def box_filter(hi, s):
    """uint8 [..., s H, s W, 3] -> uint8 [..., H, W, 3]: per channel (sum of the s x s block + s s / 2) / (s s) in
    integers."""
    hi = np.asarray(hi)
    assert hi.dtype == np.uint8 and hi.shape[-3] % s == 0 and hi.shape[-2] % s == 0 and hi.shape[-1] == 3
    lead, H, W = hi.shape[:-3], hi.shape[-3] // s, hi.shape[-2] // s
    blocks = hi.reshape(lead + (H, s, W, s, 3)).astype(np.int64)
    total = blocks.sum(axis=(-4, -2))
    return ((total + (s * s) // 2) // (s * s)).astype(np.uint8)


# the four free views of the GPU test: eyes relative to the table centre at table height, all looking at the point 5 cm
# above the table centre; 120 x 160 pixels, f = 0.9 W, principal point at the centre of the image
VIEW_H, VIEW_W = 120, 160
VIEW_EYES = [((0.9, -0.9, 0.7), (0.0, 0.0, 1.0)), ((-0.2, 1.1, 0.5), (0.0, 0.0, 1.0)),
             ((0.0, 0.0, 1.3), (1.0, 0.0, 0.0)), ((1.2, 0.1, 0.25), (0.0, 0.0, 1.0))]


def free_views(cfg, table_z, height=VIEW_H, width=VIEW_W):
    """The four perception.Camera objects for a world of config ``cfg`` whose table top is at ``table_z``."""
    centre = np.array([cfg.table_center[0], cfg.table_center[1], table_z], dtype=np.float64)
    cams = []
    for eye, up in VIEW_EYES:
        cam = look_at(centre + np.array(eye), centre + np.array([0.0, 0.0, 0.05]), up=up, height=height, width=width)
        f = 0.9 * width
        cam.set_calibration([[f, 0.0, 0.5 * (width - 1)], [0.0, f, 0.5 * (height - 1)], [0.0, 0.0, 1.0]], None, None)
        cams.append(cam)
    return cams
