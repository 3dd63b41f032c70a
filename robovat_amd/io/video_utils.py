"""Frames to files with what is installed: Pillow and NumPy.

The reference's PushEnv hands its screenshots to ``cv2.VideoWriter`` with the XVID codec (``push_env.py:282-327,
1155-1162``).  Neither cv2 nor any other video encoder (imageio, av, ffmpeg) is a dependency here, so ``FrameWriter``
writes what Pillow and NumPy can, chosen by the extension of the path:

  ``.png``  an animated PNG -- lossless, and every browser plays it
  ``.gif``  an animated GIF -- palette-quantised by Pillow, for places that take nothing else
  ``.npz``  ``frames`` uint8 [T, H, W, 3] and ``fps``, compressed -- for code

``.avi`` and every other extension is a ValueError.  ``read_frames`` reads the three back.

Pillow merges a frame that equals its predecessor into it and adds the durations up.  A writer here gives every frame the
same whole number of milliseconds (``frame_ms``; GIF: a multiple of 10) and ``read_frames`` repeats a decoded frame
duration / frame_ms times, so a recording in which nothing moves for a while still has the number of frames that were
appended.  ``frame_ms``, the count and the rate travel in the file (PNG text chunks, the GIF comment) so that reading does not
depend on the caller knowing the rate.
"""
import os

import numpy as np

EXTENSIONS = ('.png', '.gif', '.npz')


def _as_frame(frame):
    if hasattr(frame, 'detach'):
        frame = frame.detach().cpu().numpy()
    a = np.asarray(frame)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError('a frame is uint8 [H, W, 3], got %s %s' % (a.dtype, tuple(a.shape)))
    return np.ascontiguousarray(a)


class FrameWriter(object):
    """``FrameWriter(path, fps)``; ``append(frame)`` (uint8 [H, W, 3], NumPy or torch) or ``extend(frames)``; ``close()``
    writes the file -- the three formats are written in one piece, so the frames are kept in host memory until then -- and
    returns the path, or None when no frame was appended (no file then).  Also a context manager."""

    def __init__(self, path, fps):
        self.path = str(path)
        self.ext = os.path.splitext(self.path)[1].lower()
        if self.ext not in EXTENSIONS:
            raise ValueError('FrameWriter writes %s, not %r' % (' / '.join(EXTENSIONS), self.ext))
        self.fps = float(fps)
        if not self.fps > 0.0:
            raise ValueError('FrameWriter: fps must be positive')
        step = 10 if self.ext == '.gif' else 1      # (a GIF counts hundredths of a second; below 20 ms players slow down)
        self.frame_ms = max(2 * step if self.ext == '.gif' else 1, int(round(1000.0 / self.fps / step)) * step)
        self.frames = []
        self.closed = False

    def __len__(self):
        return len(self.frames)

    def append(self, frame):
        if self.closed:
            raise ValueError('FrameWriter: %s is closed' % self.path)
        a = _as_frame(frame)
        if self.frames and a.shape != self.frames[0].shape:
            raise ValueError('FrameWriter: a frame of %s after frames of %s' % (tuple(a.shape), tuple(self.frames[0].shape)))
        self.frames.append(a.copy())

    def extend(self, frames):
        if hasattr(frames, 'detach'):
            frames = frames.detach().cpu().numpy()
        for f in frames:
            self.append(f)

    def close(self):
        if self.closed:
            return self.path if self.frames else None
        self.closed = True
        if not self.frames:
            return None
        d = os.path.dirname(os.path.abspath(self.path))
        if not os.path.isdir(d):
            os.makedirs(d)
        if self.ext == '.npz':
            np.savez_compressed(self.path, frames=np.stack(self.frames), fps=np.float64(self.fps))
            return self.path
        from PIL import Image
        images = [Image.fromarray(f) for f in self.frames]
        note = 'frame_ms=%d frames=%d fps_milli=%d' % (self.frame_ms, len(images), int(round(1000.0 * self.fps)))
        if self.ext == '.png':
            from PIL import PngImagePlugin
            info = PngImagePlugin.PngInfo()
            info.add_text('robovat_amd', note)
            images[0].save(self.path, format='PNG', save_all=True, append_images=images[1:], duration=self.frame_ms, loop=0,
                           pnginfo=info)
        else:
            images[0].save(self.path, format='GIF', save_all=True, append_images=images[1:], duration=self.frame_ms, loop=0,
                           comment=note.encode())
        return self.path

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _note(text):
    out = {}
    for part in (text.decode() if isinstance(text, bytes) else str(text)).split():
        k, _, v = part.partition('=')
        if v.isdigit():
            out[k] = int(v)
    return out


def read_frames(path):
    """(frames uint8 [T, H, W, 3], fps) of a file ``FrameWriter`` wrote.  PNG and npz give back the bytes that were
    appended; GIF what its palette kept of them."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext == '.npz':
        with np.load(str(path)) as z:
            return z['frames'], float(z['fps'])
    if ext not in EXTENSIONS:
        raise ValueError('read_frames reads %s, not %r' % (' / '.join(EXTENSIONS), ext))
    from PIL import Image
    with Image.open(str(path)) as im:
        note = _note(im.info.get('robovat_amd' if ext == '.png' else 'comment', ''))
        frame_ms = note.get('frame_ms')
        out = []
        for k in range(getattr(im, 'n_frames', 1)):
            im.seek(k)
            a = np.asarray(im.convert('RGB'), dtype=np.uint8)
            ms = im.info.get('duration', frame_ms)
            reps = int(round(float(ms) / frame_ms)) if frame_ms and ms else 1
            out += [a] * max(reps, 1)
    if 'frames' in note and len(out) != note['frames']:
        raise ValueError('%s: decoded %d frames, the file says %d' % (path, len(out), note['frames']))
    return np.stack(out), note['fps_milli'] / 1000.0 if 'fps_milli' in note else (1000.0 / frame_ms if frame_ms else 0.0)


def contact_sheet(frames, path, every=1, columns=4, gap=2):
    """One PNG with every ``every``-th frame of ``frames`` (uint8 [T, H, W, 3]) side by side, ``columns`` per row, in
    order; the last frame is always among them.  Returns the indices of the frames shown."""
    from PIL import Image
    if hasattr(frames, 'detach'):
        frames = frames.detach().cpu().numpy()
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[3] != 3 or len(frames) == 0:
        raise ValueError('contact_sheet: frames are uint8 [T, H, W, 3], got %s %s' % (frames.dtype, tuple(frames.shape)))
    pick = list(range(0, len(frames), max(int(every), 1)))
    if pick[-1] != len(frames) - 1:
        pick.append(len(frames) - 1)
    h, w = frames.shape[1:3]
    cols = max(min(int(columns), len(pick)), 1)
    rows = (len(pick) + cols - 1) // cols
    sheet = np.full((rows * h + (rows - 1) * gap, cols * w + (cols - 1) * gap, 3), 255, dtype=np.uint8)
    for k, t in enumerate(pick):
        r, c = divmod(k, cols)
        sheet[r * (h + gap): r * (h + gap) + h, c * (w + gap): c * (w + gap) + w] = frames[t]
    Image.fromarray(sheet).save(str(path), format='PNG')
    return pick
