"""Utilities for depth images: the sensor noise model of ``robovat/perception/depth_utils.py`` on the host.

``gamma_noise``, ``gaussian_noise`` and ``threshold_gradients`` keep the reference's names and signatures and, like it,
draw from NumPy's global generator (``np.random.seed`` steers them).  They are NumPy mirrors for single images and small
batches; the batched version on the device is ``lib.World.depth_noise`` (``rv_depth_noise``), whose draws
are keyed Philox blocks instead, and ``VecGrasp4DofEnv`` applies that one when ``OBSERVATION.DEPTH_NOISE`` is set.

``resize_bicubic`` is the upsampling both share: Pillow's ``Image.resize(BICUBIC)`` of a mode-F image -- what the
reference's ``scipy.misc.imresize(..., interp='bicubic', mode='F')`` called -- restated in float32 (Pillow keeps its
weights and running sums in float64; the difference is a few units in the last place of the largest grid value).

``transform`` and ``crop`` are the reference's ``image_utils`` pair that its ``depth_utils`` re-exports: translate and
rotate an image with nearest-neighbour resampling, and cut a window out of it with zero fill.  Together they make the
grasp-centred image a grasp-quality model reads; the batched version on the device is ``lib.World.grasp_crops``
(``rv_grasp_crops``).

``inpaint`` is NOT part of this module: it fills the holes of a real sensor's image, runs a data-dependent number of
iterations, and its final resize in the reference goes through an 8-bit image.
"""
import numpy as np


def _keys(t):
    """Keys' cubic convolution kernel with a = -0.5 (support 2), float32."""
    t = np.abs(t)
    near = ((np.float32(1.5) * t - np.float32(2.5)) * t) * t + np.float32(1.0)
    far = (((t - np.float32(5.0)) * t + np.float32(8.0)) * t - np.float32(4.0)) * np.float32(-0.5)
    return np.where(t < 1, near, np.where(t < 2, far, np.float32(0.0))).astype(np.float32)


def _resize_axis(a, factor):
    """Upsample the last axis of a float32 array by the integer ``factor``."""
    f32 = np.float32
    n_in = a.shape[-1]
    n_out = n_in * factor
    center = (np.arange(n_out).astype(f32) + f32(0.5)) / f32(factor)
    first = np.maximum(((center - f32(2.0)) + f32(0.5)).astype(np.int32), 0)
    stop = np.minimum(((center + f32(2.0)) + f32(0.5)).astype(np.int32), n_in)
    count = np.minimum(stop - first, 4)
    weights = np.zeros((4, n_out), f32)
    total = np.zeros(n_out, f32)
    for k in range(4):
        live = k < count
        weights[k] = np.where(live, _keys(((first + k).astype(f32) - center) + f32(0.5)), f32(0.0))
        total = np.where(live, total + weights[k], total).astype(f32)
    out = np.zeros(a.shape[:-1] + (n_out,), f32)
    for k in range(4):
        live = k < count
        wk = np.where(live, weights[k] / np.where(live, total, f32(1.0)), f32(0.0)).astype(f32)
        out = np.where(live, out + a[..., np.minimum(first + k, n_in - 1)] * wk, out).astype(f32)
    return out


def resize_bicubic(grid, factor):
    """Upsample ``grid`` [h, w] by the integer ``factor`` as Pillow's BICUBIC resize of a mode-F image does: separable,
    the horizontal pass first with its result kept in float32, then the vertical; per output index the taps within 2 of
    its centre, normalised by their own sum (2 or 3 taps at a border).  Returns float32 [h * factor, w * factor]."""
    if int(factor) != factor or int(factor) < 1:
        raise ValueError('resize_bicubic: the factor must be a positive integer, got %r' % (factor,))
    g = np.asarray(grid, np.float32)
    if g.ndim != 2:
        raise ValueError('resize_bicubic: grid must be [h, w], got %s' % (g.shape,))
    rows = _resize_axis(g, int(factor))
    return np.ascontiguousarray(_resize_axis(np.ascontiguousarray(rows.T), int(factor)).T)


def transform(data, translation, theta):
    """The reference's ``image_utils.transform`` (``robovat/perception/image_utils.py:14-41``, re-exported by its
    ``depth_utils``): a new image [H, W] (or [H, W, C]) of the same dtype, ``data`` translated by ``translation`` = (row
    shift, column shift) and then rotated by ``theta`` radians (positive = counter-clockwise) about ``(W/2, H/2)``,
    resampled with nearest neighbour, zero outside.  Float64, defined by the inverse map: destination pixel ``(x, y)``
    reads source ``(W/2 - tx, H/2 - ty) + [[cos, -sin], [sin, cos]] (x - W/2, y - H/2)``, each coordinate rounded by
    ``floor(v + 0.5)``.  The reference calls ``cv2.warpAffine(..., INTER_NEAREST)``, which rounds its coordinates in fixed
    point; OpenCV is not available to compare with, so agreement with it on pixels whose source coordinate lies at a
    rounding boundary is UNVERIFIED.  The batched version on the device is ``lib.World.grasp_crops``."""
    data = np.asarray(data)
    if data.ndim not in (2, 3):
        raise ValueError('transform: expected an image [H, W] or [H, W, C], got %s' % (data.shape,))
    height, width = data.shape[0], data.shape[1]
    ty, tx = float(translation[0]), float(translation[1])
    c, s = np.cos(float(theta)), np.sin(float(theta))
    y, x = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing='ij')
    ox, oy = x - width / 2.0, y - height / 2.0
    sx = (width / 2.0 - tx) + (c * ox - s * oy)
    sy = (height / 2.0 - ty) + (s * ox + c * oy)
    ix, iy = np.floor(sx + 0.5), np.floor(sy + 0.5)
    inside = (ix >= 0) & (ix < width) & (iy >= 0) & (iy < height)
    ix = np.where(inside, ix, 0).astype(np.int64)
    iy = np.where(inside, iy, 0).astype(np.int64)
    out = data[iy, ix]
    out[~inside] = 0
    return out.astype(data.dtype)


def crop(data, height, width, c0=None, c1=None):
    """The reference's ``image_utils.crop`` (``robovat/perception/image_utils.py:44-86``): the ``height`` x ``width``
    window of ``data`` [H, W] (or [H, W, C]) centred on row ``c0`` and column ``c1`` (None: the image centre), rows
    ``floor(c0 - height / 2)`` to ``floor(c0 + height / 2)`` and columns likewise, zero where the window leaves the image
    (what PIL's ``crop`` does); same dtype.  ValueError when the two floors do not span ``height`` x ``width``, as there."""
    data = np.asarray(data)
    if data.ndim not in (2, 3):
        raise ValueError('crop: expected an image [H, W] or [H, W, C], got %s' % (data.shape,))
    height = int(np.round(height))
    width = int(np.round(width))
    if c0 is None:
        c0 = float(data.shape[0]) / 2
    if c1 is None:
        c1 = float(data.shape[1]) / 2
    r0 = int(np.floor(c0 - float(height) / 2))
    r1 = int(np.floor(c0 + float(height) / 2))
    q0 = int(np.floor(c1 - float(width) / 2))
    q1 = int(np.floor(c1 + float(width) / 2))
    if r1 - r0 != height or q1 - q0 != width:
        raise ValueError('Crop dims are incorrect.')
    out = np.zeros((height, width) + data.shape[2:], data.dtype)
    a0, a1 = max(r0, 0), min(r1, data.shape[0])
    b0, b1 = max(q0, 0), min(q1, data.shape[1])
    if a1 > a0 and b1 > b0:
        out[a0 - r0:a1 - r0, b0 - q0:b1 - q0] = data[a0:a1, b0:b1]
    return out


def threshold_gradients(data, threshold):
    """Zero every pixel of the depth image ``data`` [H, W] whose gradient magnitude (central differences of the float32
    image, one-sided at the border) exceeds ``threshold``.  Returns a new array."""
    out = np.array(data, copy=True)
    d0, d1 = np.gradient(out.astype(np.float32))
    magnitude = np.sqrt(d0.astype(np.float64) ** 2 + d1.astype(np.float64) ** 2)
    out[magnitude > threshold] = 0.0
    return out


def _as_batch(data):
    data = np.asarray(data)
    if data.ndim not in (3, 4):
        raise ValueError('expected an image [H, W, C] or a batch [N, H, W, C], got %s' % (data.shape,))
    return data if data.ndim == 4 else data[np.newaxis]


def gamma_noise(data, gamma_shape=1000):
    """Multiply each image of ``data`` ([H, W, C] or [N, H, W, C]) by one Gamma(gamma_shape, 1 / gamma_shape) sample
    (mean 1).  Returns float64, as the reference does."""
    images = _as_batch(data)
    samples = np.random.gamma(gamma_shape, 1.0 / gamma_shape, size=images.shape[0])
    out = images * samples.reshape(-1, 1, 1, 1)
    return out if np.ndim(data) == 4 else out[0]


def gaussian_noise(data, prob=0.5, rescale_factor=4.0, sigma=0.005):
    """Add correlated Gaussian noise to channel 0 of each image of ``data`` ([H, W, C] or [N, H, W, C]): with probability
    ``prob`` a grid of N(0, sigma^2) values of 1 / ``rescale_factor`` the image's size, upsampled by ``resize_bicubic``
    and added where the image is > 0.  ``rescale_factor`` must be an integer that divides the image size (the reference
    breaks otherwise).  Returns [H, W, 1] or [N, H, W, 1] in the dtype of ``data``; ``data`` itself is left alone."""
    images = _as_batch(data)
    factor = int(rescale_factor)
    height, width = images.shape[1], images.shape[2]
    if factor != rescale_factor or factor < 1 or height % factor or width % factor:
        raise ValueError('gaussian_noise: rescale_factor must be an integer dividing the image size %d x %d' % (height, width))
    out = []
    for i in range(images.shape[0]):
        image = np.array(images[i, :, :, 0], copy=True)
        if np.random.rand() < prob:
            coarse = np.random.normal(scale=sigma, size=(height // factor) * (width // factor))
            noise = resize_bicubic(coarse.reshape(height // factor, width // factor), factor)
            hit = image > 0
            image[hit] += noise[hit].astype(image.dtype)
        out.append(image[:, :, np.newaxis])
    out = np.stack(out)
    return out if np.ndim(data) == 4 else out[0]
