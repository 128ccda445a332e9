"""Parameter carriers for ``PatchPipeline(chain=[...])``.

The classes have the names and constructor arguments of the reference's transforms (mmlf/data/hci4d.py:416-1090) and the
type rules of its asserts, but they are NOT callable on data: they carry parameters, say which slot of the fused chain
they fill and draw their random numbers from Python's ``random`` stream exactly as the reference's ``__call__`` would.
``mmlf_amd.patches`` validates a list of them against the slot order and runs it as one gather on the device.

Slot order (anything else is a ValueError naming the offending element):

    [scale] [shear] RandomCrop(n[, pad]) [CenterCrop(ps)] [Rotate90 | RandomRotate]
    [RedistColor] [Brightness] [Contrast] [Noise]
"""
import numpy as np

SLOTS = ('scale', 'shear', 'crop', 'center', 'rotate', 'color', 'brightness', 'contrast', 'noise')


def _need(value, types, what):
    # bool is an int to isinstance; the reference's `assert isinstance(x, int)` lets it through, a chain should not
    if isinstance(value, bool) or not isinstance(value, types):
        names = types.__name__ if isinstance(types, type) else ' or '.join(t.__name__ for t in types)
        raise TypeError(f'{what} must be {names}, found {type(value).__name__} {value!r}')


def _size(size, what):
    """int or (h, w), as hci4d.py:546-552 / 590-595 / 633-638; stored as the reference stores it: a tuple"""
    if isinstance(size, tuple):
        if len(size) != 2:
            raise ValueError(f'{what}: a tuple size has two entries, found {size!r}')
        for s in size:
            _need(s, int, f'{what} size entry')
        return size
    _need(size, int, f'{what} size')
    return (size, size)


class Transform:
    slot = None

    def draw(self, rng):
        """this transform's draws from `rng` in the reference's call order; a dict of plain numbers"""
        return {}

    def __repr__(self):
        args = ', '.join(f'{k}={v!r}' for k, v in vars(self).items())
        return f'{type(self).__name__}({args})'


# ---------------------------------------------------------------------------------------------- scale
class DownSampling(Transform):
    """frame[..., ::factor, ::factor]; gt and mpi[:, 4] divided by float(factor) (hci4d.py:483-510)"""
    slot = 'scale'

    def __init__(self, factor):
        _need(factor, int, 'DownSampling factor')
        if factor < 1:
            raise ValueError(f'DownSampling factor must be >= 1, found {factor}')
        self.factor = factor

    def draw(self, rng):
        return dict(down=self.factor)


class RandomDownSampling(Transform):
    """DownSampling(random.randint(1, max_factor)) (hci4d.py:513-530)"""
    slot = 'scale'

    def __init__(self, max_factor=4):
        _need(max_factor, int, 'RandomDownSampling max_factor')
        if max_factor < 1:
            raise ValueError(f'RandomDownSampling max_factor must be >= 1, found {max_factor}')
        self.max_factor = max_factor

    def draw(self, rng):
        return dict(down=rng.randint(1, self.max_factor))


class Zoom(Transform):
    """scipy.ndimage.zoom(order=0) of the last two axes; gt and mpi[:, 4] times float(factor) (hci4d.py:416-457)"""
    slot = 'scale'

    def __init__(self, factor):
        _need(factor, float, 'Zoom factor')
        if not factor > 0.0:
            raise ValueError(f'Zoom factor must be positive, found {factor}')
        self.factor = factor

    def draw(self, rng):
        return dict(zoom=self.factor)


class RandomZoom(Transform):
    """Zoom(random.uniform(min_scale, max_scale)) (hci4d.py:460-480)"""
    slot = 'scale'

    def __init__(self, min_scale=0.5, max_scale=1.0):
        _need(min_scale, (float, int), 'RandomZoom min_scale')
        _need(max_scale, (float, int), 'RandomZoom max_scale')
        if not (min_scale > 0 and max_scale > 0):
            raise ValueError(f'RandomZoom scales must be positive, found ({min_scale}, {max_scale})')
        self.interval = (min_scale, max_scale)

    def draw(self, rng):
        return dict(zoom=rng.uniform(self.interval[0], self.interval[1]))


def zoom_size(n, factor):
    """output extent of scipy.ndimage.zoom for an axis of n: int(round(n * factor)), Python's round"""
    return int(round(n * factor))


def zoom_map(n_in, n_out):
    """source index of every output index of scipy.ndimage.zoom(order=0), as Zoom calls it (mode='constant', cval=0,
    grid_mode=False): the output grid's end points sit on the input's, floor(c + 0.5) with c = o * ((n_in - 1) /
    (n_out - 1)) in double, the ratio formed first as scipy forms it.  Where c lands past n_in - 1 -- the LAST index of
    about 3 % of the (n_in, n_out) pairs, where the rounded ratio times n_out - 1 exceeds n_in - 1 by one ulp, 15 -> 26
    for one -- scipy writes its constant, zero, and not the last sample: that entry is -1 here, and the gather writes
    zero for it.  The reference's patches have that zero row and column; so have these."""
    if n_out < 1 or n_in < 1:
        raise ValueError(f'zoom of an axis of {n_in} to {n_out}')
    if n_out == 1:
        return np.zeros(1, np.int32)
    ratio = float(n_in - 1) / float(n_out - 1)
    c = np.arange(n_out, dtype=np.float64) * ratio
    src = np.floor(c + 0.5).astype(np.int32)
    src[c > n_in - 1] = -1
    return src


def down_map(n_in, factor):
    """source index of every output index of a[::factor]"""
    return np.arange(0, n_in, factor, dtype=np.int32)


# ---------------------------------------------------------------------------------------------- shear
class Shift(Transform):
    """two-tap circular shear of the four stacks by disp * (view - views // 2); gt and mpi[:, 4] minus float(disp)
    (hci4d.py:894-990)"""
    slot = 'shear'

    def __init__(self, disp):
        _need(disp, float, 'Shift disp')
        self.disp = disp

    def draw(self, rng):
        return dict(disp=self.disp)


class RandomShift(Transform):
    """Shift(random.uniform(*disp_range)); a float r > 0 means (-r, r) (hci4d.py:993-1028)"""
    slot = 'shear'

    def __init__(self, disp_range):
        if isinstance(disp_range, tuple):
            if len(disp_range) != 2:
                raise ValueError(f'RandomShift disp_range has two entries, found {disp_range!r}')
            for d in disp_range:
                _need(d, (float, int), 'RandomShift disp_range entry')
            self.disp_range = disp_range
        else:
            _need(disp_range, float, 'RandomShift disp_range')
            if not disp_range > 0:
                raise ValueError(f'RandomShift disp_range must be positive, found {disp_range}')
            self.disp_range = (-disp_range, disp_range)

    def draw(self, rng):
        return dict(disp=rng.uniform(self.disp_range[0], self.disp_range[1]))


class IntegerShift(Transform):
    """circular roll of the four stacks by disp * (view - views // 2) whole pixels, the I stack's second axis the other
    way; gt and mpi[:, 4] minus float(disp) (hci4d.py:821-891)"""
    slot = 'shear'

    def __init__(self, disp):
        _need(disp, int, 'IntegerShift disp')
        self.disp = disp

    def draw(self, rng):
        return dict(idisp=self.disp)


# ---------------------------------------------------------------------------------------------- crops
class RandomCrop(Transform):
    """a size x size window at random.randint(pad, extent - size - pad), y first (hci4d.py:620-664)"""
    slot = 'crop'

    def __init__(self, size, pad=0):
        self.size = _size(size, 'RandomCrop')
        _need(pad, int, 'RandomCrop pad')
        if pad < 0:
            raise ValueError(f'RandomCrop pad must be >= 0, found {pad}')
        self.pad = pad


class CenterCrop(Transform):
    """the centred size x size window, offset int((extent - size) / 2) (hci4d.py:580-617)"""
    slot = 'center'

    def __init__(self, size):
        self.size = _size(size, 'CenterCrop')


# ---------------------------------------------------------------------------------------------- rotation
class Rotate90(Transform):
    """one quarter turn with the stacks re-labelled (hci4d.py:1031-1070); the mask is not rotated"""
    slot = 'rotate'

    def draw(self, rng):
        return dict(rot=1)


class RandomRotate(Transform):
    """random.randint(0, 3) quarter turns (hci4d.py:1073-1087)"""
    slot = 'rotate'

    def draw(self, rng):
        return dict(rot=rng.randint(0, 3))


# ---------------------------------------------------------------------------------------------- colour
class RedistColor(Transform):
    """a random 3x3 matrix with unit row and column sums on the colour channels (hci4d.py:667-716)"""
    slot = 'color'

    def draw(self, rng):
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
        return dict(mat=mat)


class Brightness(Transform):
    """images times random.uniform(-level, level) + 1 (hci4d.py:754-785)"""
    slot = 'brightness'

    def __init__(self, level=0.9):
        _need(level, float, 'Brightness level')
        self.level = level

    def draw(self, rng):
        return dict(bright=rng.uniform(-self.level, self.level) + 1.0)


class Contrast(Transform):
    """x * alpha + mean(H stack) * (1 - alpha), alpha = random.uniform(-level, level) + 1 (hci4d.py:719-751)"""
    slot = 'contrast'

    def __init__(self, level=0.9):
        _need(level, float, 'Contrast level')
        self.level = level

    def draw(self, rng):
        return dict(contrast=rng.uniform(-self.level, self.level) + 1.0)


class Noise(Transform):
    """independent N(0, stdev^2) samples on the four stacks and the centre view (hci4d.py:788-818).  The reference draws
    them from NumPy's global generator, so nothing is taken from ``random`` here; the device draws them from a
    counter-based generator of its own (``PatchPipeline(noise_seed=...)``), which is NOT NumPy's stream."""
    slot = 'noise'

    def __init__(self, stdev=0.01):
        _need(stdev, float, 'Noise stdev')
        if stdev < 0.0:
            raise ValueError(f'Noise stdev must be >= 0, found {stdev}')
        self.stdev = stdev
