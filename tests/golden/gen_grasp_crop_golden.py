"""Generate tests/golden/grasp_crop_golden.json by RUNNING the reference's perception/image_utils.crop (build container
only).

    python tests/golden/gen_grasp_crop_golden.py

gen_golden.py is imported for the stubs it installs (pybullet, cv2, gym, easydict, the numpy-1 names).  ``crop`` goes
through Pillow, which is here.  The reference's ``transform`` CANNOT be run: it calls ``cv2.getRotationMatrix2D`` and
``cv2.warpAffine``, and OpenCV is not available (cv2 is one of the stubs), so there is no golden for it -- the tests
check ``depth_utils.transform`` on cases with a known answer instead, and its agreement with OpenCV on pixels whose
source coordinate lies at a rounding boundary stays unverified.  Only DATA is written: the images, the windows and the
reference's outputs.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_golden  # noqa: E402,F401  (the stubs)

from robovat.perception import image_utils  # noqa: E402

F = np.float32
# (height, width, c0, c1) per image shape: inside the image, leaving it on each of the four sides, larger than the image,
# the default centre, odd and even sizes, a fractional centre and sizes that np.round takes to the next integer
WINDOWS = {
    (12, 16): [(4, 6, None, None), (5, 7, None, None), (4, 6, 5.0, 7.0), (5, 5, 6.5, 8.25), (6, 4, 1.0, 8.0),
               (6, 4, 11.0, 8.0), (4, 6, 6.0, 1.0), (4, 6, 6.0, 15.0), (6, 6, 0.0, 0.0), (6, 6, 12.0, 16.0),
               (20, 24, None, None), (16, 8, None, 3.0), (3.6, 4.4, 6.0, 8.0), (1, 1, 0.0, 15.0)],
    (11, 15): [(4, 6, None, None), (5, 7, None, None), (7, 9, None, None), (5, 7, 5.0, 7.0), (6, 4, 0.5, 7.5),
               (6, 4, 10.5, 7.5), (4, 6, 5.5, 0.5), (4, 6, 5.5, 14.5), (15, 21, None, None), (12, 16, 5.5, 7.5),
               (3, 3, 10.0, 14.0), (2.5, 3.5, 5.5, 7.5)],
}


def f32_list(a):
    """float32 values as the shortest decimals that read back to the same float32"""
    return [float(str(v)) for v in np.asarray(a, F).reshape(-1)]


def main():
    rng = np.random.default_rng(20261020)
    cases = []
    for (height, width), windows in WINDOWS.items():
        image = (0.5 + rng.random((height, width))).astype(F)
        for h, w, c0, c1 in windows:
            out = image_utils.crop(image, h, w, c0, c1)
            assert out.dtype == F
            cases.append({'image_height': height, 'image_width': width, 'image': f32_list(image),
                          'height': h, 'width': w, 'c0': c0, 'c1': c1,
                          'out_shape': list(out.shape), 'out': f32_list(out)})
        touched = [c for c in cases if c['image_height'] == height and 0.0 in c['out']]
        assert len(touched) >= 6, 'the windows that leave the image carry zeros'
    with open(os.path.join(HERE, 'grasp_crop_golden.json'), 'w') as f:
        json.dump({'cases': cases}, f, sort_keys=True, separators=(',', ':'))
        f.write('\n')


if __name__ == '__main__':
    main()
