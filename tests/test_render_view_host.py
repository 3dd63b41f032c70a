"""The host side of rv_render_view and of recording, without a GPU: perception.look_at / camera_row, the
camera row of a supersampled image and the box filter the GPU test compares with (tests/render_view_host.py),
io.video_utils.FrameWriter, and what lib.view_params refuses."""
import numpy as np
import pytest

from robovat_amd import abi, configs, lib
from robovat_amd.io import video_utils
from robovat_amd.perception import camera_row, look_at

import camera_host as ch
import render_view_host as rvh


def _project(row, p):
    """float64 pixel (u, v) of world point p through a calibration row [17]"""
    row = np.asarray(row, dtype=np.float64)
    fx, fy, cx, cy, sk = row[:5]
    pc = row[5:14].reshape(3, 3) @ np.asarray(p, dtype=np.float64) + row[14:17]
    return np.array([(fx * pc[0] + sk * pc[1]) / pc[2] + cx, fy * pc[1] / pc[2] + cy]), pc[2]


@pytest.mark.parametrize('eye,up', [((1.5, -0.9, 0.7), (0, 0, 1)), ((0.4, 1.1, 0.5), (0, 0, 1)), ((0.6, 0.0, 1.3), (1, 0, 0)),
                                    ((1.8, 0.1, 0.25), (0, 1, 1))])
def test_look_at(eye, up):
    """the target projects to the centre of the image, in front of the camera; the rotation is orthonormal and right
    handed; the image's down direction opposes `up`; the camera sits at `eye`"""
    target = np.array([0.6, 0.0, 0.05])
    cam = look_at(eye, target, up=up, height=120, width=160, fov_y_deg=50.0)
    assert (cam.height, cam.width) == (120, 160)
    R = np.asarray(cam.rotation, dtype=np.float64)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-6) and np.isclose(np.linalg.det(R), 1.0, atol=1e-6)      # (Camera keeps float32)
    (u, v), z = _project(camera_row(cam).astype(np.float64), target)
    assert abs(u - 79.5) < 1e-4 and abs(v - 59.5) < 1e-4 and z > 0          # (the row is float32)
    assert np.allclose(np.asarray(cam.pose.position), eye, atol=1e-6)
    assert R[1] @ np.asarray(up, dtype=np.float64) < 0                      # image y (down) against up
    # a point above the target (along up) lands higher in the image; the vertical field of view is fov_y_deg
    (_, v_up), _ = _project(camera_row(cam), target + 0.05 * np.asarray(up, dtype=np.float64))
    assert v_up < v
    assert np.isclose(2 * np.degrees(np.arctan(0.5 * 120 / cam.intrinsics[1, 1])), 50.0)
    assert cam.intrinsics[0, 0] == cam.intrinsics[1, 1] and cam.intrinsics[0, 1] == 0


def test_look_at_refuses_degenerate_views():
    with pytest.raises(ValueError):
        look_at((0, 0, 1), (0, 0, 1))
    with pytest.raises(ValueError):
        look_at((0, 0, 1), (0, 0, 0), up=(0, 0, 1))
    with pytest.raises(ValueError):
        look_at((1, 0, 1), (0, 0, 0), fov_y_deg=180.0)


def test_camera_row_round_trip():
    """camera_row is the inverse of camera_host.camera_of: row -> Camera -> row gives the float32 row back exactly, and
    Camera -> row -> Camera keeps the calibration to float32 rounding"""
    cfg = configs.make_rv_config(n_envs=1)
    cfg.cam_height, cfg.cam_width = 120, 160
    cam = look_at((1.5, -0.9, 0.7), (0.6, 0.0, 0.05), height=120, width=160)
    cam.set_calibration([[144.0, 0.25, 79.5], [0.0, 143.5, 59.5], [0, 0, 1]], None, None)      # (with a skew)
    row = camera_row(cam)
    assert row.dtype == np.float32 and row.shape == (17,)
    assert list(row[:5]) == [144.0, 143.5, 79.5, 59.5, 0.25]
    back = ch.camera_of(cfg, row)
    assert np.array_equal(camera_row(back), row)
    assert np.allclose(back.intrinsics, cam.intrinsics) and np.allclose(back.rotation, cam.rotation, atol=1e-7)
    assert np.allclose(back.translation, cam.translation, atol=1e-6) and (back.height, back.width) == (120, 160)


@pytest.mark.parametrize('s', [1, 2, 3, 4])
def test_scaled_row_maps_pixels(s):
    """pixel (u, v) of a world point in the base view lies at (s u + (s - 1) / 2, s v + (s - 1) / 2) in the view of the
    scaled row: the s x s block of output pixel (u, v) is centred on it.  (Intrinsics chosen so that the float32 products
    are exact; the rest is float64 rounding.)"""
    cam = look_at((1.5, -0.9, 0.7), (0.6, 0.0, 0.05), height=24, width=32)
    cam.set_calibration([[28.75, 0.5, 15.5], [0.0, 29.25, 11.5], [0, 0, 1]], None, None)
    row = camera_row(cam)
    hi = rvh.scaled_row(row, s)
    assert hi.dtype == np.float32 and np.array_equal(hi[5:], row[5:])
    assert list(hi[:5]) == [s * 28.75, s * 29.25, s * 15.5 + (s - 1) / 2, s * 11.5 + (s - 1) / 2, s * 0.5]
    for p in ([0.6, 0.0, 0.05], [0.45, 0.2, 0.0], [0.8, -0.3, 0.1]):
        (u, v), _ = _project(row, p)
        (U, V), _ = _project(hi, p)
        assert abs(U - (s * u + (s - 1) / 2)) < 1e-9 and abs(V - (s * v + (s - 1) / 2)) < 1e-9
    assert np.array_equal(rvh.scaled_row(np.stack([row, row]), s), np.stack([hi, hi]))


def test_box_filter_on_a_hand_made_image():
    """(sum + s s / 2) / (s s) per channel in integers: rounds half up, keeps 0 and 255, blocks do not leak"""
    hi = np.zeros((4, 6, 3), np.uint8)
    hi[0:2, 0:2] = [[[0, 1, 255], [0, 1, 255]], [[0, 1, 255], [1, 2, 255]]]      # sums 1, 5, 1020 -> 0, 1, 255
    hi[0:2, 2:4] = [[[1, 3, 7], [1, 3, 7]], [[0, 3, 7], [0, 3, 8]]]              # sums 2, 12, 29 -> 1 (half up), 3, 7
    hi[2:4, 4:6] = 200
    want = np.zeros((2, 3, 3), np.uint8)
    want[0, 0], want[0, 1], want[1, 2] = [0, 1, 255], [1, 3, 7], [200, 200, 200]
    assert np.array_equal(rvh.box_filter(hi, 2), want)
    assert np.array_equal(rvh.box_filter(hi, 1), hi)
    rng = np.random.RandomState(3)
    for s in (3, 4):
        img = rng.randint(0, 256, (2, 2 * s, 3 * s, 3)).astype(np.uint8)
        got = rvh.box_filter(img, s)
        assert got.shape == (2, 2, 3, 3)
        for k in range(2):
            for r in range(2):
                for c in range(3):
                    block = img[k, r * s:(r + 1) * s, c * s:(c + 1) * s].reshape(-1, 3).astype(int)
                    assert list(got[k, r, c]) == [(int(block[:, ch_].sum()) + s * s // 2) // (s * s) for ch_ in range(3)]


def _frames(t=7, h=9, w=11, seed=0):
    """frames with repeats (a recording in which nothing moves for a while) and full-range bytes"""
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 256, (4, h, w, 3)).astype(np.uint8)
    return base[[0, 1, 1, 1, 2, 3, 3][:t]]


@pytest.mark.parametrize('ext', ['.png', '.npz'])
@pytest.mark.parametrize('fps', [30, 24.0, 7])
def test_frame_writer_round_trip_is_lossless(tmp_path, ext, fps):
    """animated PNG and npz give back every frame that was appended, repeats included, bit for bit, and the rate"""
    frames = _frames()
    path = str(tmp_path / 'sub' / ('clip' + ext))
    with video_utils.FrameWriter(path, fps) as wr:
        wr.append(frames[0])
        wr.extend(frames[1:])
        assert len(wr) == 7
    got, rate = video_utils.read_frames(path)
    assert got.dtype == np.uint8 and np.array_equal(got, frames) and rate == float(fps)


def test_frame_writer_gif(tmp_path):
    """GIF: the frame count and the size (the palette may change bytes)"""
    frames = _frames()
    wr = video_utils.FrameWriter(str(tmp_path / 'clip.gif'), 25)
    wr.extend(frames)
    path = wr.close()
    got, rate = video_utils.read_frames(path)
    assert got.shape == frames.shape and rate == 25.0
    from PIL import Image
    with Image.open(path) as im:
        assert im.format == 'GIF' and im.size == (11, 9)


def test_frame_writer_refusals_and_empty(tmp_path):
    for name in ('clip.avi', 'clip.mp4', 'clip'):
        with pytest.raises(ValueError):
            video_utils.FrameWriter(str(tmp_path / name), 30)
    with pytest.raises(ValueError):
        video_utils.FrameWriter(str(tmp_path / 'clip.png'), 0)
    wr = video_utils.FrameWriter(str(tmp_path / 'none.png'), 30)
    assert wr.close() is None and not (tmp_path / 'none.png').exists()
    wr = video_utils.FrameWriter(str(tmp_path / 'a.png'), 30)
    wr.append(np.zeros((4, 5, 3), np.uint8))
    for bad in (np.zeros((4, 6, 3), np.uint8), np.zeros((4, 5, 3), np.float32), np.zeros((4, 5), np.uint8)):
        with pytest.raises(ValueError):
            wr.append(bad)
    wr.close()
    with pytest.raises(ValueError):
        wr.append(np.zeros((4, 5, 3), np.uint8))


def test_contact_sheet(tmp_path):
    frames = _frames()
    pick = video_utils.contact_sheet(frames, str(tmp_path / 'sheet.png'), every=3, columns=2, gap=1)
    assert pick == [0, 3, 6]
    from PIL import Image
    with Image.open(str(tmp_path / 'sheet.png')) as im:
        sheet = np.asarray(im.convert('RGB'))
    assert sheet.shape == (2 * 9 + 1, 2 * 11 + 1, 3)
    assert np.array_equal(sheet[:9, :11], frames[0]) and np.array_equal(sheet[:9, 12:], frames[3])
    assert np.array_equal(sheet[10:, :11], frames[6]) and (sheet[10:, 12:] == 255).all()
    assert video_utils.contact_sheet(frames, str(tmp_path / 's2.png'), every=4) == [0, 4, 6]      # the last frame is kept


def test_view_params():
    p = lib.view_params(3, 120, 160)
    assert (p.n_views, p.height, p.width, p.supersample) == (3, 120, 160, 1)
    p = lib.view_params(abi.RV_VIEW_MAX_VIEWS, abi.RV_VIEW_MAX_SIDE, 1, abi.RV_VIEW_MAX_SUPERSAMPLE)
    assert (p.n_views, p.height, p.width, p.supersample) == (4096, 4096, 1, 4)
    for bad in (dict(n_views=0), dict(n_views=4097), dict(height=0), dict(height=4097), dict(width=0), dict(width=-1),
                dict(width=4097), dict(supersample=0), dict(supersample=5), dict(height=12.5), dict(supersample=True)):
        kw = dict(n_views=1, height=8, width=8, supersample=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            lib.view_params(**kw)


def test_view_params_is_the_header_struct():
    import ctypes as C
    assert C.sizeof(abi.rv_view_params) == 16 and [n for n, _ in abi.rv_view_params._fields_] == ['n_views', 'height', 'width', 'supersample']
    assert 'rv_render_view' in lib.SYMBOLS and 'rv_render_view' in abi.VIEW_API


def test_recording_is_off_without_the_key():
    """a config without RECORDING, or with USE false, makes no recorder"""
    from robovat_amd.envs import recording

    class Env(object):
        pass
    e = Env()
    e.config = configs.push_env_config()
    assert 'RECORDING' not in e.config and recording.make_recorder(e) is None
    e.config = configs.push_env_config(RECORDING={'USE': False})
    assert recording.make_recorder(e) is None
