"""Writes tests/golden/randaug_lut.npz: inputs and the REFERENCE's own outputs of the six table operations of
data/utils/randaugment.py (autocontrast_func, equalize_func, brightness_func, contrast_func, solarize_func,
posterize_func) at the arguments of m = 7 and m = 2.  tests/test_randaug_cpu.py holds augment.RandAugment's restatement
against them, bit for bit.

    python tools/gen_randaug_golden.py /path/to/reference

The reference file is loaded by path and is not copied anywhere; only its outputs are stored.  It imports cv2 at the
top, which this tool does not need to be installed: a stand-in module registered under that name provides the three calls
the table functions make (split, merge, calcHist with float32 counts of shape [bins, 1], as cv2 returns them).  The warp
and filter functions (warpAffine, filter2D, getRotationMatrix2D) need the real cv2 and are NOT pinned this way: the
stand-in raises if they are reached.

Posterize: the reference writes ``np.uint8(255 << (8 - bits))``, which numpy 2 refuses for a Python integer above 255
(numpy 1 wrapped it to the low byte).  The tool hands ``bits`` over as ``np.int64``: numpy casts its own scalars with that
wrap-around, so the reference function runs unchanged and computes what it computed under numpy 1.

AutoContrast inputs: every channel of the stored inputs contains the value 0 or is constant.  The reference computes
``offset = -low * scale`` with ``low`` a numpy uint8 scalar, so for low > 0 the negation wraps (``-np.uint8(5)`` is 251)
and its table is not PIL's, although its docstring promises "same output as PIL.ImageOps.autocontrast".  DESIGN.md 4i
follows PIL there and says so; with low = 0 the two agree, and that is what can be pinned.  The tool checks that the
wrap is still there (it reports the count of differing values on one input with low > 0), so a fixed reference would be
noticed.
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (7, 2)


def cv2_stand_in():
    cv2 = types.ModuleType('cv2')

    def split(img):
        return [np.ascontiguousarray(img[:, :, c]) for c in range(img.shape[2])]

    def merge(channels):
        return np.stack(channels, axis=2)

    def calcHist(images, channels, mask, hist_size, ranges):
        assert len(images) == 1 and channels == [0] and mask is None and hist_size == [256] and list(ranges) == [0, 256]
        return np.bincount(images[0].reshape(-1), minlength=256).astype(np.float32).reshape(256, 1)

    def missing(*a, **k):
        raise RuntimeError('this needs the real cv2: warps and filters are not pinned by this tool')

    cv2.split, cv2.merge, cv2.calcHist = split, merge, calcHist
    cv2.warpAffine = cv2.filter2D = cv2.getRotationMatrix2D = missing
    cv2.INTER_LINEAR = 1
    return cv2


def load_reference(root):
    sys.modules['cv2'] = cv2_stand_in()
    spec = importlib.util.spec_from_file_location('reference_randaugment', os.path.join(root, 'data', 'utils', 'randaugment.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs():
    """Seven images, at most 40 x 50: random, narrow-range with 0 present, four-level, gradient, a tiny one (Equalize's
    step is 0), one with a constant channel."""
    rng = np.random.RandomState(20260)
    ims = [rng.randint(0, 256, (17, 13, 3)).astype(np.uint8),
           rng.randint(0, 256, (29, 23, 3)).astype(np.uint8)]
    narrow = rng.randint(0, 150, (19, 21, 3)).astype(np.uint8)          # hi < 255: a scale that is not 1
    narrow[..., 1] = narrow[..., 1] // 2
    ims.append(narrow)
    ims.append((rng.randint(0, 4, (40, 50, 3)) * 67).astype(np.uint8))   # four levels: 0, 67, 134, 201
    yy, xx = np.mgrid[0:37, 0:41]
    ims.append(np.stack([(3 * xx + yy) % 200, (xx * yy) % 97, (5 * yy + 2 * xx) % 256], axis=2).astype(np.uint8))
    ims.append(rng.randint(0, 256, (7, 5, 3)).astype(np.uint8))
    const = rng.randint(0, 256, (13, 11, 3)).astype(np.uint8)
    const[..., 0] = 91                                                   # constant channel: hi <= lo
    ims.append(const)
    for im in ims:                       # see the docstring: a channel's minimum is 0 unless the channel is constant
        for c in range(3):
            if im[..., c].min() != im[..., c].max():
                im[0, 0, c] = 0
    return ims


def main():
    ref = load_reference(sys.argv[1])
    ims = inputs()
    out = {'n_images': np.int64(len(ims)), 'levels': np.array(LEVELS, dtype=np.int64)}
    for i, im in enumerate(ims):
        out[f'in{i}'] = im
        out[f'autocontrast{i}'] = ref.autocontrast_func(im)
        out[f'equalize{i}'] = ref.equalize_func(im)
        for m in LEVELS:
            (factor,) = ref.arg_dict['Brightness'](m)
            (thresh,) = ref.arg_dict['Solarize'](m)
            (bits,) = ref.arg_dict['Posterize'](m)
            out[f'args_m{m}'] = np.array([factor, thresh, bits], dtype=np.float64)
            out[f'brightness{i}_m{m}'] = ref.brightness_func(im, factor)
            out[f'contrast{i}_m{m}'] = ref.contrast_func(im, ref.arg_dict['Contrast'](m)[0])
            out[f'solarize{i}_m{m}'] = ref.solarize_func(im, thresh)
            out[f'posterize{i}_m{m}'] = ref.posterize_func(im, np.int64(bits))
    for k, v in out.items():
        assert v.dtype in (np.uint8, np.int64, np.float64), (k, v.dtype)
    # the uint8 wrap of the reference's AutoContrast offset, on an input whose minimum is not 0
    probe = (np.random.RandomState(1).randint(40, 200, (16, 16, 3))).astype(np.uint8)
    with np.errstate(over='ignore'):
        got = ref.autocontrast_func(probe)
    pil = np.empty_like(probe)
    for c in range(3):
        lo, hi = int(probe[..., c].min()), int(probe[..., c].max())
        scale = 255.0 / (hi - lo)
        pil[..., c] = (np.arange(256) * scale + (-lo * scale)).clip(0, 255).astype(np.uint8)[probe[..., c]]
    print(f'AutoContrast with low > 0: {int((got != pil).sum())} of {got.size} values differ from the PIL definition')
    path = os.path.join(ROOT, 'tests', 'golden', 'randaug_lut.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {os.path.getsize(path)} bytes, {len(out)} arrays')


if __name__ == '__main__':
    main()
