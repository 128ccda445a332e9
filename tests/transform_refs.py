"""numpy restatement of every transform a PatchPipeline chain can hold (reference mmlf/data/hci4d.py:416-1090), on the data
tuple (h, v, i, d, center, gt, mpi, mask, index) of hci4d.py:272-293.  It is the CPU yardstick of the chain tests, held
itself to the reference's recorded outputs (tests/golden/g12_patch_chain.npz, written by tests/golden/make_golden_chain.py):
the goldens cover a handful of draws, this covers any.  Draws come from Python's `random` in the reference's call order.

A chain is written as a list of (class name, positional arguments): CASES below is shared by the golden script (which
instantiates the REFERENCE's classes from it), by this module and by the tests (which instantiate mmlf_amd.transforms).
"""
import math
import random as _random

import numpy as np

F32 = np.float32
NAMES = ('h', 'v', 'i', 'd', 'center', 'gt', 'mpi', 'mask')
PS, VIEWS, PLANES, SAMPLES = 8, 3, 2, 3
EVEN, ODD = (40, 52), (41, 53)

# tag -> (scene seed, frame, chain)
CASES = {
    # train/cli.py:78-87 (a 40-row frame holds the 24-px crop at factor 1 only)
    'cli': (1, ODD, [('RandomDownSampling', (1,)), ('RandomShift', (1.0,)), ('RandomCrop', (PS + 16,)), ('CenterCrop', (PS,)),
                     ('RandomRotate', ()), ('RedistColor', ()), ('Brightness', ()), ('Contrast', ())]),
    'cli_plain': (2, EVEN, [('RandomCrop', (PS + 16,)), ('CenterCrop', (PS,))]),
    # every factor of the interval leaves 9 rows for the 8-px crop; the shear's taps reach 3 px into a 9 x 12 frame
    'rzoom_shift': (3, EVEN, [('RandomZoom', (0.213, 0.237)), ('RandomShift', (2.0,)), ('RandomCrop', (PS,))]),
    # 41 * 0.5 = 20.5 and 53 * 0.5 = 26.5: Python's round goes to the even neighbour, 20 x 26
    'zoom_half_odd': (4, ODD, [('Zoom', (0.5,)), ('RandomCrop', (PS,))]),
    'zoom_up': (5, EVEN, [('Zoom', (1.3,)), ('RandomShift', (1.0,)), ('RandomCrop', (PS + 16,)), ('CenterCrop', (PS,)),
                          ('RandomRotate', ())]),
    'down_ishift': (6, ODD, [('DownSampling', (3,)), ('IntegerShift', (2,)), ('RandomCrop', (PS,))]),
    'ishift_neg': (7, EVEN, [('IntegerShift', (-2,)), ('RandomCrop', (PS,)), ('RandomRotate', ())]),
    # a 10 x 13 frame, an 8-px crop and taps 1..3 px away: every sample wraps
    'shift_wrap': (8, EVEN, [('DownSampling', (4,)), ('RandomShift', ((1.5, 2.5),)), ('RandomCrop', (PS,))]),
    'rot90': (9, ODD, [('Shift', (0.6,)), ('RandomCrop', (PS,)), ('Rotate90', ())]),
    'crop_pad': (10, EVEN, [('RandomCrop', (PS, 3))]),
    'bright_contrast': (11, EVEN, [('RandomCrop', (PS,)), ('Brightness', (0.3,)), ('Contrast', (0.5,))]),
    'color_bright_contrast': (12, ODD, [('RandomCrop', (PS,)), ('RedistColor', ()), ('Brightness', (0.3,)),
                                        ('Contrast', (0.5,))]),
}


def case_seed(tag, k):
    return 1000 * (list(CASES).index(tag) + 1) + k


def build(namespace, chain):
    """the chain's objects from a module or class namespace (mmlf_amd.transforms, the reference's hci4d)"""
    return [getattr(namespace, name)(*args) for name, args in chain]


def _spatial(a):
    return a.ndim >= 2 and a.shape[-1] > 1 and a.shape[-2] > 1


def _scale_disparity(data, op, value):
    data[5] = op(data[5], F32(value))
    data[6] = data[6].copy()
    data[6][:, 4] = op(data[6][:, 4], F32(value))


def zoom_index(n_in, n_out):
    """scipy.ndimage.zoom(order=0, mode='constant'): (source index, filled) per output index.  The coordinate is
    c = o * ((n_in - 1) / (n_out - 1)) in double and the index floor(c + 0.5); where c > n_in - 1 (rounding can push the
    last one there) scipy writes its constant 0 and no sample."""
    ratio = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    c = np.arange(n_out) * ratio
    fill = c > n_in - 1
    return np.where(fill, 0, np.floor(c + 0.5)).astype(np.int64), fill


def tf_zoom(data, factor):
    """Zoom, hci4d.py:429-457"""
    data = list(data)
    for k in range(len(data)):
        if _spatial(data[k]):
            h, w = data[k].shape[-2:]
            (ym, yfill), (xm, xfill) = zoom_index(h, int(round(h * factor))), zoom_index(w, int(round(w * factor)))
            data[k] = data[k][..., ym[:, None], xm[None, :]]
            data[k][..., yfill, :] = 0
            data[k][..., :, xfill] = 0
    _scale_disparity(data, np.multiply, factor)
    return tuple(data)


def tf_downsample(data, factor):
    """DownSampling, hci4d.py:495-510"""
    data = list(data)
    for k in range(len(data)):
        if _spatial(data[k]):
            data[k] = data[k][..., ::factor, ::factor]
    _scale_disparity(data, np.divide, factor)
    return tuple(data)


def _roll(a, s, axis):
    """cat([a[-s:], a[:-s]]) with Python's slice clamping: |s| >= the extent (and s = 0) leave `a` as it is"""
    return a if s == 0 or abs(s) >= a.shape[axis] else np.roll(a, s, axis)


def tf_shift(data, disp):
    """Shift, hci4d.py:907-990: per view two rolls blended with float32 weights; W first, then H, the I stack's H the other
    way"""
    data = list(data)
    h, v, i, d = (a.copy() for a in data[:4])
    views = h.shape[-4]
    half = int(views / 2)
    for n in range(views):
        alpha, s0 = math.modf(disp * (n - half))
        alpha = abs(alpha)
        s1 = int(s0 + math.copysign(1.0, s0))
        s0 = int(s0)
        w0, w1 = F32(1.0 - alpha), F32(alpha)

        def blend(a, axis, sign):
            return _roll(a, sign * s0, axis) * w0 + _roll(a, sign * s1, axis) * w1
        h[n] = blend(h[n], -1, 1)
        v[n] = blend(v[n], -2, 1)
        i[n] = blend(blend(i[n], -1, 1), -2, -1)
        d[n] = blend(blend(d[n], -1, 1), -2, 1)
    data[:4] = h, v, i, d
    _scale_disparity(data, np.subtract, disp)
    return tuple(data)


def tf_integer_shift(data, disp):
    """IntegerShift, hci4d.py:843-891"""
    data = list(data)
    h, v, i, d = (a.copy() for a in data[:4])
    views = h.shape[-4]
    half = int(views / 2)
    for n in range(views):
        s = disp * (n - half)
        h[n] = _roll(h[n], s, -1)
        v[n] = _roll(v[n], s, -2)
        i[n] = _roll(_roll(i[n], s, -1), -s, -2)
        d[n] = _roll(_roll(d[n], s, -1), s, -2)
    data[:4] = h, v, i, d
    _scale_disparity(data, np.subtract, float(disp))
    return tuple(data)


def tf_crop(data, size, pos):
    """Crop, hci4d.py:566-577"""
    (y, x) = pos
    return tuple(a[..., y:y + size, x:x + size] if _spatial(a) else a for a in data)


def tf_rotate90(data):
    """Rotate90, hci4d.py:1055-1070 (entries 0..6: the mask, entry 7, is not rotated)"""
    data = list(data)
    for k in range(7):
        data[k] = np.flip(np.swapaxes(data[k], -1, -2), -2).copy()
    data[0], data[1] = data[1], np.flip(data[0], -4)
    data[2], data[3] = data[3], np.flip(data[2], -4)
    return tuple(data)


def draw_color_matrix(rng):
    """hci4d.py:682-692"""
    mat = np.zeros((3, 3))
    mat[0, 0] = rng.uniform(0.0, 1.0)
    mat[0, 1] = rng.uniform(0.0, 1.0 - mat[0, 0])
    mat[1, 0] = rng.uniform(0.0, 1.0 - mat[0, 0])
    mat[1, 1] = rng.uniform(0.0, 1.0 - max(mat[0, 1], mat[1, 0]))
    mat[0, 2] = 1.0 - mat[0, 0] - mat[0, 1]
    mat[1, 2] = 1.0 - mat[1, 0] - mat[1, 1]
    mat[2, 0] = 1.0 - mat[0, 0] - mat[1, 0]
    mat[2, 1] = 1.0 - mat[0, 1] - mat[1, 1]
    mat[2, 2] = mat[0, 0] + mat[0, 1] + mat[1, 0] + mat[1, 1] - 1.0
    return mat


def tf_redist_color(data, mat):
    """RedistColor, hci4d.py:694-714: float64 matrix entries times float32 images, every step rounded to float32"""
    data = list(data)
    for k in range(5):
        src = data[k].astype(np.float64)
        out = np.empty(data[k].shape, np.float32)
        for r in range(3):
            acc = (mat[r, 0] * src[..., 0, :, :]).astype(np.float32)
            acc = (acc.astype(np.float64) + mat[r, 1] * src[..., 1, :, :]).astype(np.float32)
            acc = (acc.astype(np.float64) + mat[r, 2] * src[..., 2, :, :]).astype(np.float32)
            out[..., r, :, :] = acc
        data[k] = out
    return tuple(data)


def tf_brightness(data, alpha):
    """Brightness, hci4d.py:776-783"""
    data = list(data)
    for k in range(5):
        data[k] = data[k] * F32(alpha)
    return tuple(data)


def tf_contrast(data, alpha):
    """Contrast, hci4d.py:741-749: the mean of the horizontal stack as it stands"""
    data = list(data)
    mean = data[0].mean()
    for k in range(5):
        data[k] = data[k] * F32(alpha) + mean * F32(1.0 - alpha)
    return tuple(data)


def tf_noise(data, stdev, generator):
    """Noise, hci4d.py:811-816 with a numpy Generator / RandomState given: float32 += float64"""
    data = list(data)
    for k in range(5):
        data[k] = (data[k].astype(np.float64) + generator.normal(scale=stdev, size=data[k].shape)).astype(np.float32)
    return tuple(data)


def apply_chain(scene, chain, rng=None, generator=None):
    """one sample of `chain` (a list of (name, args)) from `scene`, drawing from `rng` as the reference would"""
    rng = rng or _random
    data = tuple(np.array(a, copy=True) for a in scene)
    for name, args in chain:
        if name == 'Zoom':
            data = tf_zoom(data, args[0])
        elif name == 'RandomZoom':
            data = tf_zoom(data, rng.uniform(*args))
        elif name == 'DownSampling':
            data = tf_downsample(data, args[0])
        elif name == 'RandomDownSampling':
            data = tf_downsample(data, rng.randint(1, args[0]))
        elif name == 'Shift':
            data = tf_shift(data, args[0])
        elif name == 'RandomShift':
            lo, hi = args[0] if isinstance(args[0], tuple) else (-args[0], args[0])
            data = tf_shift(data, rng.uniform(lo, hi))
        elif name == 'IntegerShift':
            data = tf_integer_shift(data, args[0])
        elif name == 'RandomCrop':
            size, pad = args[0], (args[1] if len(args) > 1 else 0)
            h, w = data[0].shape[-2:]
            assert h > size and w > size
            y = rng.randint(pad, h - size - pad)
            x = rng.randint(pad, w - size - pad)
            data = tf_crop(data, size, (y, x))
        elif name == 'CenterCrop':
            h, w = data[0].shape[-2:]
            data = tf_crop(data, args[0], (int((h - args[0]) / 2), int((w - args[0]) / 2)))
        elif name == 'Rotate90':
            data = tf_rotate90(data)
        elif name == 'RandomRotate':
            for _ in range(rng.randint(0, 3)):
                data = tf_rotate90(data)
        elif name == 'RedistColor':
            data = tf_redist_color(data, draw_color_matrix(rng))
        elif name == 'Brightness':
            level = args[0] if args else 0.9
            data = tf_brightness(data, rng.uniform(-level, level) + 1.0)
        elif name == 'Contrast':
            level = args[0] if args else 0.9
            data = tf_contrast(data, rng.uniform(-level, level) + 1.0)
        elif name == 'Noise':
            data = tf_noise(data, args[0] if args else 0.01, generator)
        else:
            raise ValueError(name)
    return data
