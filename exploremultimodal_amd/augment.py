"""The image views of a sample from decoded pixels (data/utils/transforms.py: RandomResizedCropAndInterpolationWithTwoPic,
then the flip, ToTensor and Normalize / map_pixels of data/base_dataset.py, which the reference runs on the CPU with PIL).

One random crop box per image is resampled twice: antialiased bicubic to ``size`` for the patch embedding (``image``) and
Lanczos to ``second_size`` for the dVAE (``image4dalle``); a second, independent box gives ``image_aug``.  The sources of
a batch differ in size, so they travel packed in one byte buffer (``pack_images``).  A device buffer goes through
hip.crop_resample (csrc/augment.hip: two launches per batch); a CPU buffer takes a torch restatement of the same
definition, which is what the tests compare the kernels with.  No autograd: this is input preparation.

Stated difference from PIL: values stay fp32 between the two passes and at the end and are not clamped to [0, 255]; PIL
rounds to uint8 after each pass, so its image is this one rounded.

``RandAugment`` (data/utils/randaugment.py: RandomAugment, which the reference runs with numpy and cv2 on the full-size
source) goes in front of the crop: it maps a packed batch to a packed batch of the same layout.  A device buffer goes
through hip.randaug (csrc/randaug.hip), a CPU buffer through the torch restatement of DESIGN.md 4i further down.
"""
import math

import torch

from . import hip
from .dvae import logit_laplace_eps

BICUBIC, LANCZOS = hip.FILTER_BICUBIC, hip.FILTER_LANCZOS
_RADIUS = {BICUBIC: 2.0, LANCZOS: 3.0}
_PAD = 16           # packed buffers are a multiple of this many bytes long (the kernel reads whole aligned dwords)


def pack_images(images, pin_memory=False):
    """[uint8 [H, W, 3] tensors] -> {'pixels': uint8 [nbytes], 'table': ((byte offset, H, W), ...)}: what a collate
    function returns.  Images are laid end to end without padding between them, so an image or a row may start on any
    byte.  The table is plain Python: it stays on the host when DataLoaderX uploads the batch.
    The buffer is pageable unless ``pin_memory=True``: a collate function runs in the DataLoader's worker processes, where
    a pinned allocation would open the GPU (after a fork it cannot; after a spawn every worker would), and a tensor that
    comes back from a worker is no longer pinned anyway.  DataLoaderX pins on the consumer side before it uploads; ask for
    a pinned buffer only in the process that owns the GPU."""
    table, off = [], 0
    for i, im in enumerate(images):
        if not torch.is_tensor(im) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            raise ValueError(f'pack_images: image {i} must be a uint8 [H, W, 3] tensor, got '
                             f'{tuple(im.shape) if torch.is_tensor(im) else type(im).__name__}')
        H, W = int(im.shape[0]), int(im.shape[1])
        if H < 1 or W < 1:
            raise ValueError(f'pack_images: image {i} is empty ({H} x {W})')
        table.append((off, H, W))
        off += H * W * 3
    total = max(_PAD, (off + _PAD - 1) // _PAD * _PAD)
    pixels = torch.zeros(total, dtype=torch.uint8, pin_memory=bool(pin_memory))
    for (o, H, W), im in zip(table, images):
        pixels[o:o + H * W * 3] = im.reshape(-1)
    return {'pixels': pixels, 'table': tuple(table)}


def unpack_image(packed, i):
    """Image i of a packed batch as a uint8 [H, W, 3] view."""
    o, H, W = _table(packed)[i]
    return packed['pixels'][o:o + H * W * 3].view(H, W, 3)


def _table(packed):
    t = packed['table']
    if torch.is_tensor(t):          # a tensor table works too, at the price of a device-to-host read when it was uploaded
        t = t.tolist()
    return [(int(o), int(H), int(W)) for o, H, W in t]


def _checked_pack(packed, who):
    """(pixels, table) of a packed batch, after the refusals that every consumer makes in the name ``who``: a contiguous 1-D
    uint8 buffer, at least one image, every image inside the buffer, a device buffer as the kernels need it."""
    pixels, table = packed['pixels'], _table(packed)
    if pixels.dtype != torch.uint8 or pixels.dim() != 1 or not pixels.is_contiguous():
        raise ValueError(f'{who}: packed["pixels"] must be a contiguous 1-D uint8 buffer (3 channels, HWC)')
    if not table:
        raise ValueError(f'{who}: empty batch')
    for i, (o, H, W) in enumerate(table):
        if H < 1 or W < 1 or o < 0 or o + H * W * 3 > pixels.numel():
            raise ValueError(f'{who}: image {i} (offset {o}, {H} x {W} x 3) is not inside the packed buffer')
    if pixels.is_cuda and (pixels.numel() % 4 or pixels.data_ptr() % 4):
        raise ValueError(f'{who}: the device buffer must be 4-byte aligned and a multiple of 4 bytes long (pack_images '
                         'pads it)')
    return pixels, table


def sample_crop_params(sizes, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), generator=None):
    """torchvision's RandomResizedCrop.get_params for every (H, W) of ``sizes`` -> int64 [N, 4] boxes (top, left, h, w).
    Up to 10 tries of area fraction ~ U(scale) times aspect ratio w / h log-uniform in ``ratio``, the first box that fits
    wins and is placed uniformly; after 10 misses the largest centred box whose ratio is clamped into ``ratio``.  The same
    seeded ``generator`` gives the same boxes."""
    if not (0 < scale[0] <= scale[1]) or not (0 < ratio[0] <= ratio[1]):
        raise ValueError(f'sample_crop_params: need 0 < min <= max for scale {scale} and ratio {ratio}')
    lo, hi = math.log(ratio[0]), math.log(ratio[1])

    def uniform(a, b):
        return torch.empty(1).uniform_(a, b, generator=generator).item()

    def below(n):
        return int(torch.randint(0, n, (1,), generator=generator).item())

    boxes = []
    for H, W in sizes:
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError(f'sample_crop_params: empty image {H} x {W}')
        box = None
        for _ in range(10):
            target = H * W * uniform(scale[0], scale[1])
            aspect = math.exp(uniform(lo, hi))
            w = int(round(math.sqrt(target * aspect)))
            h = int(round(math.sqrt(target / aspect)))
            if 0 < w <= W and 0 < h <= H:
                box = (below(H - h + 1), below(W - w + 1), h, w)
                break
        if box is None:
            box = fallback_box(H, W, ratio)
        boxes.append(box)
    return torch.tensor(boxes, dtype=torch.int64).reshape(-1, 4)


def fallback_box(H, W, ratio):
    """The centred box sample_crop_params falls back to: the whole image if its ratio W / H lies in ``ratio``, else the
    largest box at the nearest allowed ratio."""
    r = W / H
    if r < ratio[0]:
        w, h = W, min(H, max(1, int(round(W / ratio[0]))))
    elif r > ratio[1]:
        h, w = H, min(W, max(1, int(round(H * ratio[1]))))
    else:
        h, w = H, W
    return ((H - h) // 2, (W - w) // 2, h, w)


# ---------------------------------------------------------------------------------- the definition, restated in torch

def filter_weight(filt, x):
    """Bicubic: the Keys kernel with a = -0.5; Lanczos: sinc(x) sinc(x / 3) for |x| < 3.  x: fp64 tensor."""
    x = x.abs()
    if filt == BICUBIC:
        near = (1.5 * x - 2.5) * x * x + 1.0
        far = ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0
        return torch.where(x < 1.0, near, torch.where(x < 2.0, far, torch.zeros_like(x)))
    return torch.where(x < 3.0, torch.sinc(x) * torch.sinc(x / 3.0), torch.zeros_like(x))


def resample_matrix(n, S, filt):
    """(fp32 [S, n], fp32 [S]): row o holds the weights of output o over the n inputs of one axis (zero outside its
    window), and their sum, by which the pass divides its result.  Weights in fp64, rounded once, as the kernels do."""
    scale = n / S
    fs = max(scale, 1.0)
    support = _RADIUS[filt] * fs
    center = (torch.arange(S, dtype=torch.float64) + 0.5) * scale
    k0 = (center - support + 0.5).trunc().clamp(min=0)
    k1 = (center + support + 0.5).trunc().clamp(max=n)
    k = torch.arange(n, dtype=torch.float64)
    inside = (k[None, :] >= k0[:, None]) & (k[None, :] < k1[:, None])
    w = torch.where(inside, filter_weight(filt, (k[None, :] + 0.5 - center[:, None]) / fs), torch.zeros((), dtype=torch.float64))
    return w.float(), w.float().sum(1)


def _crop_resample_cpu(crop, S, filt, flip, mul, add):
    """crop uint8 [h, w, 3] -> fp32 [3, S, S]: horizontal pass, vertical pass, flip, value * mul[c] + add[c]."""
    wh, sh = resample_matrix(crop.shape[1], S, filt)
    wv, sv = resample_matrix(crop.shape[0], S, filt)
    t = torch.einsum('ok,ykc->yoc', wh, crop.float()) / sh[None, :, None]        # [h, S, 3]
    v = torch.einsum('oy,yxc->cox', wv, t) / sv[None, :, None]                   # [3, S, S]
    if flip:
        v = v.flip(2)
    return v * mul[:, None, None] + add[:, None, None]


class TwoViewCrop:
    """``tv = TwoViewCrop(size, second_size, mean, std)``; ``tv(packed, generator=None)`` -> {'image': fp32 [N, 3, size,
    size] (bicubic, (v / 255 - mean) / std), 'image4dalle': fp32 [N, 3, second_size, second_size] (Lanczos, map_pixels(v /
    255))} of one random box and flip per image, plus 'image_aug' (bicubic, normalised, ``size``) from a second,
    independent box and flip with ``aug_view=True``.  ``packed``: pack_images' result, on the host or uploaded.
    ``tv.apply(packed, boxes, flips, aug_boxes, aug_flips)`` is the deterministic form.
    Limits (include/vlmo_hip.h: vlmo_crop_resample): 1 <= size <= 1024, crop sides <= 8192, boxes inside their images,
    at most 65536 views per call."""

    def __init__(self, size, second_size, mean, std, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), hflip=0.5, aug_view=False):
        for n, s in (('size', size), ('second_size', second_size)):
            if not isinstance(s, int) or not 1 <= s <= hip.CROP_MAX_SIZE:
                raise ValueError(f'TwoViewCrop: {n} must be an integer in [1, {hip.CROP_MAX_SIZE}], got {s!r}')
        mean, std = [float(m) for m in mean], [float(s) for s in std]
        if len(mean) != 3 or len(std) != 3 or min(std) <= 0:
            raise ValueError('TwoViewCrop: mean and std must have 3 entries, std positive')
        if not 0.0 <= hflip <= 1.0:
            raise ValueError('TwoViewCrop: hflip is a probability')
        self.size, self.second_size, self.mean, self.std = size, second_size, mean, std
        self.scale, self.ratio, self.hflip, self.aug_view = scale, ratio, hflip, aug_view

    def _draw(self, sizes, generator):
        boxes = sample_crop_params(sizes, self.scale, self.ratio, generator)
        flips = torch.rand(len(sizes), generator=generator) < self.hflip
        return boxes, flips

    def __call__(self, packed, generator=None):
        sizes = [(H, W) for _, H, W in _table(packed)]
        boxes, flips = self._draw(sizes, generator)
        aug = self._draw(sizes, generator) if self.aug_view else (None, None)
        return self.apply(packed, boxes, flips, *aug)

    def _jobs(self, table, boxes, flips, S, filt, finish, what):
        boxes = torch.as_tensor(boxes).reshape(-1, 4).tolist()
        flips = torch.as_tensor(flips).reshape(-1).tolist()
        if len(boxes) != len(table) or len(flips) != len(table):
            raise ValueError(f'TwoViewCrop.apply: {what}: one box and one flip per image expected '
                             f'({len(table)} images, {len(boxes)} boxes, {len(flips)} flips)')
        jobs = []
        for i, ((_, H, W), (top, left, h, w)) in enumerate(zip(table, boxes)):
            top, left, h, w = int(top), int(left), int(h), int(w)
            if h < 1 or w < 1 or h > hip.CROP_MAX_SIDE or w > hip.CROP_MAX_SIDE:
                raise ValueError(f'TwoViewCrop.apply: {what} {i}: crop sides must lie in [1, {hip.CROP_MAX_SIDE}] (h={h}, w={w})')
            if top < 0 or left < 0 or top + h > H or left + w > W:
                raise ValueError(f'TwoViewCrop.apply: {what} {i}: box (top {top}, left {left}, h {h}, w {w}) is not inside '
                                 f'the {H} x {W} image')
            jobs.append((i, top, left, h, w, bool(flips[i]), S, filt, finish))
        return jobs

    def apply(self, packed, boxes, flips, aug_boxes=None, aug_flips=None):
        pixels, table = _checked_pack(packed, 'TwoViewCrop.apply')
        if (aug_boxes is None) != (aug_flips is None):
            raise ValueError('TwoViewCrop.apply: aug_boxes and aug_flips go together')
        views = [('image', self._jobs(table, boxes, flips, self.size, BICUBIC, hip.FINISH_NORMALIZE, 'box')),
                 ('image4dalle', self._jobs(table, boxes, flips, self.second_size, LANCZOS, hip.FINISH_MAP_PIXELS, 'box'))]
        if aug_boxes is not None:
            views.append(('image_aug', self._jobs(table, aug_boxes, aug_flips, self.size, BICUBIC, hip.FINISH_NORMALIZE,
                                                  'aug box')))
        if sum(len(j) for _, j in views) > hip.CROP_MAX_JOBS:
            raise ValueError(f'TwoViewCrop.apply: more than {hip.CROP_MAX_JOBS} views in one call: split the batch')
        out = {name: torch.empty(len(jobs), 3, jobs[0][6], jobs[0][6], dtype=torch.float32, device=pixels.device)
               for name, jobs in views}
        if pixels.is_cuda:
            hip.crop_resample(pixels, table, [job + (out[name][q],) for name, jobs in views for q, job in enumerate(jobs)],
                              self.mean, self.std, logit_laplace_eps)
            return out
        std = torch.tensor(self.std)
        finish = {hip.FINISH_NORMALIZE: (1.0 / (255.0 * std), -torch.tensor(self.mean) / std),
                  hip.FINISH_MAP_PIXELS: (torch.full((3,), (1 - 2 * logit_laplace_eps) / 255.0), torch.full((3,), logit_laplace_eps))}
        for name, jobs in views:
            for q, (i, top, left, h, w, flip, S, filt, fin) in enumerate(jobs):
                o, H, W = table[i]
                crop = pixels[o:o + H * W * 3].view(H, W, 3)[top:top + h, left:left + w]
                out[name][q] = _crop_resample_cpu(crop, S, filt, flip, *finish[fin])
        return out


# ------------------------------------------------------------------------------------------------------- RandAugment

PRETRAIN_AUGS = ('Identity', 'AutoContrast', 'Equalize', 'Brightness', 'Sharpness', 'ShearX', 'ShearY', 'TranslateX',
                 'TranslateY', 'Rotate')
ALL_AUGS = PRETRAIN_AUGS + ('Solarize', 'Posterize', 'Contrast')
AUG_CODES = {'Identity': hip.AUG_IDENTITY, 'AutoContrast': hip.AUG_AUTOCONTRAST, 'Equalize': hip.AUG_EQUALIZE,
             'Brightness': hip.AUG_BRIGHTNESS, 'Sharpness': hip.AUG_SHARPNESS, 'ShearX': hip.AUG_SHEAR_X,
             'ShearY': hip.AUG_SHEAR_Y, 'TranslateX': hip.AUG_TRANSLATE_X, 'TranslateY': hip.AUG_TRANSLATE_Y,
             'Rotate': hip.AUG_ROTATE, 'Solarize': hip.AUG_SOLARIZE, 'Posterize': hip.AUG_POSTERIZE,
             'Contrast': hip.AUG_CONTRAST}
_SIGNED = (hip.AUG_SHEAR_X, hip.AUG_SHEAR_Y, hip.AUG_TRANSLATE_X, hip.AUG_TRANSLATE_Y, hip.AUG_ROTATE)
_STATS = (hip.AUG_AUTOCONTRAST, hip.AUG_EQUALIZE, hip.AUG_CONTRAST)
MAX_LEVEL = 10


def aug_magnitude(code, m):
    """The reference's arg_dict at level m (MAX_LEVEL = 10), unsigned; 0 for the operations without an argument."""
    level = m / MAX_LEVEL
    if code in (hip.AUG_BRIGHTNESS, hip.AUG_SHARPNESS, hip.AUG_CONTRAST):
        return level * 1.8 + 0.1
    if code in (hip.AUG_SHEAR_X, hip.AUG_SHEAR_Y):
        return level * 0.3
    if code in (hip.AUG_TRANSLATE_X, hip.AUG_TRANSLATE_Y):
        return level * 10.0
    if code == hip.AUG_ROTATE:
        return level * 30
    if code == hip.AUG_SOLARIZE:
        return float(int(level * 256))
    if code == hip.AUG_POSTERIZE:
        return float(int(level * 4))
    return 0.0


def _aug_table(code, arg, img):
    """uint8 [3, 256]: the look-up table of a table operation for img uint8 [H, W, 3].  fp64 with every
    multiply and add a tensor operation of its own, so nothing is fused."""
    k = torch.arange(256, dtype=torch.float64)
    ident = torch.arange(256, dtype=torch.int64)
    if code == hip.AUG_BRIGHTNESS:
        t = (torch.arange(256, dtype=torch.float32) * torch.tensor(arg, dtype=torch.float32)).clamp(0, 255)
        return t.to(torch.uint8).expand(3, 256)
    if code == hip.AUG_SOLARIZE:
        return torch.where(k < arg, ident, 255 - ident).to(torch.uint8).expand(3, 256)
    if code == hip.AUG_POSTERIZE:
        return (ident & ((0xFF << (8 - int(arg))) & 0xFF)).to(torch.uint8).expand(3, 256)
    flat = img.reshape(-1, 3).long()
    hist = torch.stack([torch.bincount(flat[:, c], minlength=256) for c in range(3)])       # int64 [3, 256]
    npix = flat.shape[0]
    if code == hip.AUG_CONTRAST:
        means = (hist * ident).sum(1).double() / float(npix)
        mean = (0.114 * means[0] + 0.587 * means[1]) + 0.299 * means[2]
        return ((k - mean) * arg + mean).clamp(0, 255).to(torch.uint8).expand(3, 256)
    rows = []
    for c in range(3):
        present = hist[c].nonzero().reshape(-1)
        lo, hi = int(present[0]), int(present[-1])
        if code == hip.AUG_AUTOCONTRAST:
            if hi <= lo:
                rows.append(ident)
                continue
            scale = 255.0 / (hi - lo)
            rows.append((k * scale + (-lo * scale)).clamp(0, 255).long())
        else:                                                                               # Equalize
            step = (npix - int(hist[c, hi])) // 255
            if step == 0:
                rows.append(ident)
                continue
            below = hist[c].cumsum(0) - hist[c]
            rows.append(((step // 2 + below) // step).clamp(max=255))
    return torch.stack(rows).to(torch.uint8)


def _sharpness_cpu(img, factor):
    """PIL's ImageEnhance.Sharpness: blend of the image with its 3 x 3 smoothing (weights 1, centre 5, sum 13), the border
    copied, the result clamped; fp32 with the multiply and the add rounded separately."""
    H, W, _ = img.shape
    if factor == 1.0 or H < 3 or W < 3:
        return img.clone()
    p = img.to(torch.int32)
    s = 4 * p[1:-1, 1:-1]
    for dy in range(3):
        for dx in range(3):
            s = s + p[dy:H - 2 + dy, dx:W - 2 + dx]
    deg = (s + 6) // 13
    px = p[1:-1, 1:-1]
    v = deg.float() + torch.tensor(factor, dtype=torch.float32) * (px - deg).float()
    out = img.clone()
    out[1:-1, 1:-1] = v.clamp(0, 255).to(torch.uint8)
    return out


def aug_affine(code, arg, H, W):
    """(m00, m01, m10, m11, cx, cy, ox, oy) of a warp: output (x, y) samples source (m00 dx + m01 dy + ox, m10 dx + m11 dy +
    oy) with dx = x - cx, dy = y - cy.  The terms an operation does not use are exactly 1 or 0, so the value has the bits
    of the short form (x - f y, x + off, ...).  Rotate: cos and sin once, in fp64, on the host."""
    m00, m01, m10, m11, cx, cy, ox, oy = 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0
    if code == hip.AUG_SHEAR_X:
        m01 = -arg
    elif code == hip.AUG_SHEAR_Y:
        m10 = -arg
    elif code == hip.AUG_TRANSLATE_X:
        ox = arg
    elif code == hip.AUG_TRANSLATE_Y:
        oy = arg
    else:
        al, be = math.cos(math.radians(arg)), math.sin(math.radians(arg))
        m00, m01, m10, m11 = al, -be, be, al
        cx = ox = 0.5 * W
        cy = oy = 0.5 * H
    return m00, m01, m10, m11, cx, cy, ox, oy


def _warp_cpu(img, code, arg, fill):
    """Bilinear affine warp in fp64: taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) summed in this order, a tap
    outside the image reads ``fill``, out = floor(v + 0.5)."""
    H, W, _ = img.shape
    m00, m01, m10, m11, cx, cy, ox, oy = aug_affine(code, arg, H, W)
    dx = (torch.arange(W, dtype=torch.float64) - cx)[None, :]
    dy = (torch.arange(H, dtype=torch.float64) - cy)[:, None]
    sx = (m00 * dx + m01 * dy) + ox
    sy = (m10 * dx + m11 * dy) + oy
    x0, y0 = sx.floor(), sy.floor()
    fx, fy = sx - x0, sy - y0
    src = img.double()
    v = None
    for (tx, ty, w) in ((x0, y0, (1.0 - fx) * (1.0 - fy)), (x0 + 1, y0, fx * (1.0 - fy)), (x0, y0 + 1, (1.0 - fx) * fy),
                        (x0 + 1, y0 + 1, fx * fy)):
        inside = (tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)
        xi, yi = tx.clamp(0, W - 1).long(), ty.clamp(0, H - 1).long()
        tap = torch.where(inside[:, :, None], src[yi, xi], torch.tensor(float(fill), dtype=torch.float64))
        v = w[:, :, None] * tap if v is None else v + w[:, :, None] * tap
    return (v + 0.5).floor().clamp(0, 255).to(torch.uint8)


def _aug_cpu(img, code, arg, fill):
    """One operation on img uint8 [H, W, 3] -> a new uint8 [H, W, 3]."""
    if code in (hip.AUG_SKIP, hip.AUG_IDENTITY):
        return img.clone()
    if code == hip.AUG_SHARPNESS:
        return _sharpness_cpu(img, arg)
    if code in _SIGNED:
        return _warp_cpu(img, code, arg, fill)
    table = _aug_table(code, arg, img)
    return torch.stack([table[c][img[:, :, c].long()] for c in range(3)], dim=2)


class RandAugment:
    """``ra = RandAugment(n=2, m=7, augs=PRETRAIN_AUGS, fill=128, prob=0.5)``: the reference's RandomAugment(n, m, augs=...)
    on a packed batch.  ``ra(packed, generator=None)`` -> a packed batch with the same 'table' and new 'pixels' of the same
    length on the same device; ``plan = ra.sample(num_images, generator)`` and ``ra.apply(packed, plan)`` are its two halves.
    A plan is {'ops': int64 [N, n] (hip.AUG_* codes, -1 = slot skipped), 'args': float64 [N, n] (the signed argument of
    the operation: factor, shear, offset in pixels, angle in degrees, threshold, bits)}, both on the host.
    ``sample`` draws, from ``generator``, in this order: the [N, n] names (torch.randint over ``augs``), the [N, n] keep
    decisions (torch.rand < prob), the [N, n] signs (torch.rand < 0.5: negative), all row-major; the signs are drawn for every
    slot and used by the shear, translate and rotate operations.  The same seed gives the same plan; numpy's global
    stream, which the reference draws from, cannot be reproduced.
    Limits: those of TwoViewCrop.apply (contiguous 1-D uint8, 3 channels HWC, a device buffer 4-byte aligned and a
    multiple of 4 bytes long, sides <= 8192, at most 65536 images, images that do not overlap), 1 <= n <= 4.  'Color' is
    refused: a per-pixel fp32 3 x 3 product whose truncation cannot be pinned bit for bit, used by no reference config."""

    def __init__(self, n=2, m=7, augs=PRETRAIN_AUGS, fill=128, prob=0.5):
        if not isinstance(n, int) or not 1 <= n <= hip.AUG_MAX_SLOTS:
            raise ValueError(f'RandAugment: n must be an integer in [1, {hip.AUG_MAX_SLOTS}], got {n!r}')
        augs = tuple(augs)
        if not augs:
            raise ValueError('RandAugment: augs is empty')
        for name in augs:
            if name == 'Color':
                raise ValueError("RandAugment: 'Color' is not supported (its fp32 matrix product cannot be reproduced bit "
                                 'for bit, and no reference config uses it)')
            if name not in AUG_CODES:
                raise ValueError(f'RandAugment: unknown operation {name!r}; known: {", ".join(ALL_AUGS)}')
        if not (isinstance(m, (int, float)) and math.isfinite(m) and 0 <= m <= MAX_LEVEL):
            raise ValueError(f'RandAugment: m must lie in [0, {MAX_LEVEL}], got {m!r}')
        if not isinstance(fill, int) or not 0 <= fill <= 255:
            raise ValueError(f'RandAugment: fill must be an integer in [0, 255], got {fill!r}')
        if not 0.0 <= prob <= 1.0:
            raise ValueError('RandAugment: prob is a probability')
        self.n, self.m, self.augs, self.fill, self.prob = n, m, augs, fill, float(prob)

    def sample(self, num_images, generator=None):
        N = int(num_images)
        codes = torch.tensor([AUG_CODES[a] for a in self.augs], dtype=torch.int64)
        mags = torch.tensor([aug_magnitude(int(c), self.m) for c in codes], dtype=torch.float64)
        signed = torch.tensor([int(c) in _SIGNED for c in codes])
        pick = torch.randint(0, len(self.augs), (N, self.n), generator=generator)
        keep = torch.rand(N, self.n, generator=generator) < self.prob
        negative = torch.rand(N, self.n, generator=generator) < 0.5
        args = torch.where(signed[pick] & negative, -mags[pick], mags[pick])
        ops = torch.where(keep, codes[pick], torch.full_like(pick, hip.AUG_SKIP))
        return {'ops': ops, 'args': torch.where(keep, args, torch.zeros_like(args))}

    def __call__(self, packed, generator=None):
        return self.apply(packed, self.sample(len(_table(packed)), generator))

    def _check_plan(self, plan, table):
        ops = torch.as_tensor(plan['ops']).to(torch.int64).cpu()
        args = torch.as_tensor(plan['args']).to(torch.float64).cpu()
        if ops.dim() != 2 or tuple(ops.shape) != (len(table), self.n) or args.shape != ops.shape:
            raise ValueError(f'RandAugment.apply: the plan must hold ops and args of shape [{len(table)}, {self.n}] '
                             f'(got {tuple(ops.shape)} and {tuple(args.shape)})')
        if not torch.isfinite(args).all():
            raise ValueError('RandAugment.apply: non-finite argument in the plan')
        ops_l, args_l = ops.tolist(), args.tolist()
        for i, (orow, arow) in enumerate(zip(ops_l, args_l)):
            for s, (op, arg) in enumerate(zip(orow, arow)):
                if not hip.AUG_SKIP <= op <= hip.AUG_CONTRAST:
                    raise ValueError(f'RandAugment.apply: image {i} slot {s}: unknown op code {op}')
                if op == hip.AUG_POSTERIZE and not (0 <= arg <= 8 and arg == int(arg)):
                    raise ValueError(f'RandAugment.apply: image {i} slot {s}: posterize bits must be an integer in [0, 8], '
                                     f'got {arg}')
                if op in _SIGNED[:4] and abs(arg) > hip.AUG_MAX_SHIFT:
                    raise ValueError(f'RandAugment.apply: image {i} slot {s}: shear / translate argument {arg} outside '
                                     f'[-{hip.AUG_MAX_SHIFT}, {hip.AUG_MAX_SHIFT}]')
        return ops_l, args_l

    def apply(self, packed, plan):
        pixels, table = _checked_pack(packed, 'RandAugment.apply')
        if len(table) > hip.AUG_MAX_IMAGES:
            raise ValueError(f'RandAugment.apply: more than {hip.AUG_MAX_IMAGES} images in one call: split the batch')
        for i, (_, H, W) in enumerate(table):
            if H > hip.CROP_MAX_SIDE or W > hip.CROP_MAX_SIDE:
                raise ValueError(f'RandAugment.apply: image {i}: sides must be <= {hip.CROP_MAX_SIDE} ({H} x {W})')
        spans = sorted((o, o + H * W * 3) for o, H, W in table)
        if any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
            raise ValueError('RandAugment.apply: images overlap in the packed buffer')
        ops, args = self._check_plan(plan, table)
        covered = spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        if pixels.is_cuda:
            # the entry point writes the images' bytes only: the padding behind them (and gaps, if any) is zeroed here
            out = torch.empty_like(pixels)
            (out[spans[-1][1]:] if covered else out).zero_()
            a = [[math.cos(math.radians(v)) if op == hip.AUG_ROTATE else v for op, v in zip(orow, arow)]
                 for orow, arow in zip(ops, args)]
            b = [[math.sin(math.radians(v)) if op == hip.AUG_ROTATE else 0.0 for op, v in zip(orow, arow)]
                 for orow, arow in zip(ops, args)]
            hip.randaug(pixels, table, ops, a, b, self.fill, out=out)
            return {'pixels': out, 'table': packed['table']}
        out = torch.zeros_like(pixels)
        for (o, H, W), orow, arow in zip(table, ops, args):
            img = pixels[o:o + H * W * 3].view(H, W, 3)
            for op, arg in zip(orow, arow):
                img = _aug_cpu(img, op, arg, self.fill)
            out[o:o + H * W * 3] = img.reshape(-1)
        return {'pixels': out, 'table': packed['table']}
