"""exploremultimodal_amd.augment without a GPU: the definition of the two-view crop restated here in fp64,
pinned to torch's antialiased bicubic, and compared with the CPU path of TwoViewCrop.apply; crop sampling, packing and
refusals.  The restatement below shares no code with the package and is also the reference of tests/test_augment_gpu.py.

Tolerance of the package's fp32 paths against the restatement, on pixel values v / 255 in [0, 1]: 2e-5, i.e. atol = 2e-5 /
min(std) on the normalised outputs and 0.8 * 2e-5 after map_pixels, rtol = 0.  It is a worst case of fp32 accumulation, not
a measurement: a pass that sums T taps with sum |w| < 1.5 over values in [0, 1] is off by at most T * 2^-24 * 1.5, which is
1.1e-5 for T = 128 and 2e-5 for the 225 taps of the largest downscale tested (300 -> 8, Lanczos); typical error is far
below either."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from exploremultimodal_amd import augment as A

BICUBIC, LANCZOS = 0, 1
RADIUS = {BICUBIC: 2, LANCZOS: 3}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PIXEL_TOL = 2e-5
ATOL = PIXEL_TOL / min(STD)


# ---------------------------------------------------------------------------------------------- the fp64 restatement

def keys(x):
    x = abs(x)
    a = -0.5
    if x < 1:
        return ((a + 2) * x - (a + 3)) * x * x + 1
    if x < 2:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def sinc(x):
    return 1.0 if x == 0 else math.sin(math.pi * x) / (math.pi * x)


def lanczos(x):
    return sinc(x) * sinc(x / 3) if abs(x) < 3 else 0.0


def axis_weights(n, S, filt):
    """-> [(k0, normalised fp64 weights of taps k0, k0 + 1, ...)] for the S outputs of an axis of n inputs."""
    f = keys if filt == BICUBIC else lanczos
    scale = n / S
    fs = max(scale, 1.0)
    support = RADIUS[filt] * fs
    rows = []
    for o in range(S):
        center = (o + 0.5) * scale
        k0 = max(0, int(center - support + 0.5))
        k1 = min(n, int(center + support + 0.5))
        w = np.array([f((k + 0.5 - center) / fs) for k in range(k0, k1)], dtype=np.float64)
        rows.append((k0, w / w.sum()))
    return rows


def axis_matrix(n, S, filt):
    m = np.zeros((S, n), dtype=np.float64)
    for o, (k0, w) in enumerate(axis_weights(n, S, filt)):
        m[o, k0:k0 + len(w)] = w
    return m


def resample(crop, S, filt):
    """crop [h, w, 3] -> fp64 [S, S, 3]: horizontal pass, then vertical."""
    crop = np.asarray(crop, dtype=np.float64)
    t = np.einsum('ok,ykc->yoc', axis_matrix(crop.shape[1], S, filt), crop)
    return np.einsum('oy,yxc->oxc', axis_matrix(crop.shape[0], S, filt), t)


def view(src, box, flip, S, filt, finish, mean=MEAN, std=STD, eps=0.1):
    """One output view in fp64 [3, S, S]; finish 'norm': (v / 255 - mean) / std, 'dalle': (1 - 2 eps) v / 255 + eps."""
    top, left, h, w = [int(b) for b in box]
    v = resample(np.asarray(src)[top:top + h, left:left + w], S, filt)
    if flip:
        v = v[:, ::-1]
    v = v / 255.0
    if finish == 'norm':
        v = (v - np.asarray(mean, dtype=np.float64)) / np.asarray(std, dtype=np.float64)
    else:
        v = (1 - 2 * eps) * v + eps
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def reference_views(images, tv, boxes, flips, aug_boxes=None, aug_flips=None):
    """What TwoViewCrop.apply is defined to return, in fp64 numpy."""
    out = {'image': np.stack([view(im, b, f, tv.size, BICUBIC, 'norm', tv.mean, tv.std)
                              for im, b, f in zip(images, boxes, flips)]),
           'image4dalle': np.stack([view(im, b, f, tv.second_size, LANCZOS, 'dalle')
                                    for im, b, f in zip(images, boxes, flips)])}
    if aug_boxes is not None:
        out['image_aug'] = np.stack([view(im, b, f, tv.size, BICUBIC, 'norm', tv.mean, tv.std)
                                     for im, b, f in zip(images, aug_boxes, aug_flips)])
    return out


def random_image(H, W, seed):
    return torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


# ---------------------------------------------------------------------------------------------------------- filters

@pytest.mark.parametrize('h,w', [(37, 53), (5, 7)])
def test_bicubic_restatement_equals_torch_antialias(h, w):
    """A second implementation of the same windows and Keys constants.  Measured largest difference on pixel values in
    [0, 255]: 5.61e-5 for 37 x 53 -> 16 and 3.64e-5 for 5 x 7 -> 16 (torch builds its weights and sums in fp32); the
    bound is about 4 x the larger figure."""
    crop = random_image(h, w, 100 + h)
    ref = resample(crop.numpy(), 16, BICUBIC).transpose(2, 0, 1)
    got = F.interpolate(crop.permute(2, 0, 1)[None].float(), size=(16, 16), mode='bicubic', antialias=True,
                        align_corners=False)[0].double().numpy()
    err = np.abs(got - ref).max()
    print(f'{h} x {w} -> 16: max |torch - restatement| = {err:.3g}')
    assert err <= 2.2e-4          # measured 5.61e-5


@pytest.mark.parametrize('n,S', [(53, 16), (37, 8), (7, 16), (1, 5), (300, 8), (224, 224)])
def test_lanczos_weights(n, S):
    rows = axis_weights(n, S, LANCZOS)
    for k0, w in rows:
        assert k0 >= 0 and k0 + len(w) <= n and len(w) >= 1
        assert abs(w.sum() - 1) <= 1e-12
    const = np.full((n, n, 3), 137.0)
    assert np.abs(resample(const, S, LANCZOS) - 137.0).max() <= 1e-12 * 137


def test_largest_downscale_of_the_gpu_pack():
    """300 -> 8 with Lanczos: support 3 * 37.5 = 112.5 pixels to either side of the centre, 225 taps: more than one
    128-tap chunk of the kernels."""
    assert max(len(w) for _, w in axis_weights(300, 8, LANCZOS)) == 225
    assert max(len(w) for _, w in axis_weights(200, 8, LANCZOS)) == 150


@pytest.mark.parametrize('filt', [BICUBIC, LANCZOS])
def test_one_pixel_crop_fills_the_output(filt):
    px = np.array([[[3, 200, 77]]], dtype=np.uint8)
    out = resample(px, 9, filt)
    assert np.abs(out - px.astype(np.float64)).max() <= 1e-12 * 255


# --------------------------------------------------------------------------------------------------------- sampling

SIZES = [(480, 640), (640, 480), (33, 64), (7, 5), (1, 1), (100, 10), (300, 200)] * 6


def _fallback(H, W, ratio):
    r = W / H
    if r < ratio[0]:
        w, h = W, min(H, max(1, int(round(W / ratio[0]))))
    elif r > ratio[1]:
        h, w = H, min(W, max(1, int(round(H * ratio[1]))))
    else:
        h, w = H, W
    return ((H - h) // 2, (W - w) // 2, h, w)


@pytest.mark.parametrize('scale,ratio', [((0.08, 1.0), (3 / 4, 4 / 3)), ((0.5, 1.0), (3.0, 4.0)), ((0.2, 0.3), (0.5, 2.0))])
def test_sampled_boxes(scale, ratio):
    boxes = A.sample_crop_params(SIZES, scale, ratio, torch.Generator().manual_seed(5))
    assert boxes.shape == (len(SIZES), 4) and boxes.dtype == torch.int64
    n_fallback = 0
    for (H, W), (top, left, h, w) in zip(SIZES, boxes.tolist()):
        assert h >= 1 and w >= 1 and top >= 0 and left >= 0 and top + h <= H and left + w <= W
        if (top, left, h, w) == _fallback(H, W, ratio):
            n_fallback += 1
            continue
        # h and w are roundings of real sides whose area fraction and ratio lie in the ranges: each real side is within
        # half a pixel of the integer one
        assert (w - 0.5) * (h - 0.5) <= scale[1] * H * W and (w + 0.5) * (h + 0.5) >= scale[0] * H * W
        assert (w - 0.5) / (h + 0.5) <= ratio[1] and (w + 0.5) / (h - 0.5) >= ratio[0]
    if ratio == (3.0, 4.0):
        # a 100 x 10 image cannot hold half its area at w / h >= 3: the centred 3 x 10 box
        assert n_fallback >= 6 and boxes[5].tolist() == [48, 0, 3, 10]


@pytest.mark.parametrize('H,W,ratio,box', [
    (100, 10, (3.0, 4.0), (48, 0, 3, 10)),          # too tall: full width, h = round(10 / 3) = 3, centred
    (200, 30, (0.5, 2.0), (70, 0, 60, 30)),         # too tall: h = round(30 / 0.5) = 60, top = (200 - 60) // 2
    (10, 100, (0.25, 0.5), (0, 47, 10, 5)),         # too wide: full height, w = round(10 * 0.5) = 5, left = (100 - 5) // 2
    (7, 45, (3 / 4, 4 / 3), (0, 18, 7, 9)),         # too wide: w = round(7 * 4 / 3) = 9, left = (45 - 9) // 2
    (30, 40, (3 / 4, 4 / 3), (0, 0, 30, 40)),       # ratio inside the range: the whole image
    (1, 1, (3.0, 4.0), (0, 0, 1, 1)),               # round(1 / 3) = 0 is raised to the one pixel there is
])
def test_fallback_boxes_worked_by_hand(H, W, ratio, box):
    assert A.fallback_box(H, W, ratio) == box
    # a scale no box of this image can meet in 10 tries sends sample_crop_params to the fallback
    if (H, W) != (30, 40) and (H, W) != (1, 1):
        got = A.sample_crop_params([(H, W)], (0.9, 1.0), ratio, torch.Generator().manual_seed(0))
        assert got.tolist() == [list(box)]


def test_sampling_is_seeded():
    a = A.sample_crop_params(SIZES, generator=torch.Generator().manual_seed(11))
    b = A.sample_crop_params(SIZES, generator=torch.Generator().manual_seed(11))
    c = A.sample_crop_params(SIZES, generator=torch.Generator().manual_seed(12))
    assert torch.equal(a, b) and not torch.equal(a, c)


# ---------------------------------------------------------------------------------------------------------- packing

def test_pack_round_trip():
    ims = [random_image(1, 1, 1), random_image(7, 5, 2), random_image(33, 64, 3)]
    packed = A.pack_images(ims, pin_memory=False)
    assert packed['pixels'].dtype == torch.uint8 and packed['pixels'].dim() == 1 and packed['pixels'].numel() % 4 == 0
    assert packed['table'] == ((0, 1, 1), (3, 7, 5), (3 + 105, 33, 64))
    for i, im in enumerate(ims):
        assert torch.equal(A.unpack_image(packed, i), im)


class _Pixels(torch.utils.data.Dataset):
    def __len__(self):
        return 4

    def __getitem__(self, i):
        return {'pixels': random_image(3 + i, 5 + 2 * i, i), 'label': i}


def _collate_in_worker(samples):
    """What the README's collate function does, plus what the worker saw while doing it."""
    info = torch.utils.data.get_worker_info()
    packed = A.pack_images([s['pixels'] for s in samples])
    return {'packed': packed, 'label': torch.tensor([s['label'] for s in samples]),
            'in_worker': info is not None, 'pinned_in_worker': packed['pixels'].is_pinned(),
            'gpu_opened_in_worker': torch.cuda.is_initialized()}


def test_pack_images_in_a_dataloader_worker_does_not_pin(monkeypatch):
    """pack_images is a collate function: it runs in worker processes, where a pinned allocation would open the GPU.  A
    pin attempt is made to raise in the worker (the patch is inherited by the forked worker), whatever the machine."""
    def refuse(*a, **k):
        raise AssertionError('pin_memory() called in a DataLoader worker')
    real_zeros = torch.zeros

    def zeros(*a, **k):
        assert not k.get('pin_memory', False), 'pinned allocation in a DataLoader worker'
        return real_zeros(*a, **k)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)       # as on a machine with a GPU
    monkeypatch.setattr(torch.Tensor, 'pin_memory', refuse)
    monkeypatch.setattr(torch, 'zeros', zeros)
    loader = torch.utils.data.DataLoader(_Pixels(), batch_size=2, num_workers=1, collate_fn=_collate_in_worker,
                                         multiprocessing_context='fork')
    batches = list(loader)
    assert len(batches) == 2
    for b, batch in enumerate(batches):
        assert batch['in_worker'] and not batch['pinned_in_worker'] and not batch['gpu_opened_in_worker']
        assert not batch['packed']['pixels'].is_pinned()
        assert isinstance(batch['packed']['table'], tuple) and batch['label'].tolist() == [2 * b, 2 * b + 1]
        for j in range(2):
            assert torch.equal(A.unpack_image(batch['packed'], j), random_image(3 + 2 * b + j, 5 + 2 * (2 * b + j), 2 * b + j))


# -------------------------------------------------------------------------------------------- the package's CPU path

@pytest.fixture(scope='module')
def case():
    ims = [random_image(1, 1, 1), random_image(7, 5, 2), random_image(64, 48, 3), random_image(97, 131, 4)]
    boxes = [(0, 0, 1, 1), (1, 0, 5, 5), (10, 3, 37, 30), (0, 0, 97, 131)]
    flips = [True, False, True, False]
    aug_boxes = [(0, 0, 1, 1), (0, 0, 7, 5), (27, 18, 37, 30), (44, 78, 53, 53)]
    aug_flips = [False, True, False, True]
    tv = A.TwoViewCrop(16, 8, MEAN, STD, aug_view=True)
    packed = A.pack_images(ims, pin_memory=False)
    got = tv.apply(packed, boxes, flips, aug_boxes, aug_flips)
    ref = reference_views([im.numpy() for im in ims], tv, boxes, flips, aug_boxes, aug_flips)
    return tv, ims, packed, boxes, flips, got, ref


def test_cpu_path_agrees_with_the_restatement(case):
    tv, ims, packed, boxes, flips, got, ref = case
    assert set(got) == {'image', 'image4dalle', 'image_aug'}
    for name, tol in (('image', ATOL), ('image_aug', ATOL), ('image4dalle', 0.8 * PIXEL_TOL)):
        assert got[name].dtype == torch.float32 and tuple(got[name].shape) == ref[name].shape
        err = np.abs(got[name].double().numpy() - ref[name]).max()
        print(f'{name}: max |cpu path - restatement| = {err:.3g} (bound {tol:.3g})')
        assert err <= tol
    assert tuple(got['image'].shape) == (4, 3, 16, 16) and tuple(got['image4dalle'].shape) == (4, 3, 8, 8)


def test_flip_mirrors_the_columns(case):
    tv, ims, packed, boxes, flips, got, _ = case
    other = tv.apply(packed, boxes, [not f for f in flips])
    assert set(other) == {'image', 'image4dalle'}
    for name in other:
        assert torch.equal(other[name], got[name].flip(3))


def test_image4dalle_range_for_constant_images():
    ims = [torch.zeros(9, 14, 3, dtype=torch.uint8), torch.full((20, 11, 3), 255, dtype=torch.uint8)]
    tv = A.TwoViewCrop(16, 8, MEAN, STD)
    out = tv.apply(A.pack_images(ims, pin_memory=False), [(0, 0, 9, 14), (3, 2, 11, 7)], [False, True])['image4dalle']
    assert (out[0] - 0.1).abs().max().item() <= PIXEL_TOL and (out[1] - 0.9).abs().max().item() <= PIXEL_TOL
    assert out.min().item() >= 0.1 - PIXEL_TOL and out.max().item() <= 0.9 + PIXEL_TOL


def test_random_call_is_seeded_and_shaped():
    ims = [random_image(40, 60, 8), random_image(33, 21, 9)]
    packed = A.pack_images(ims, pin_memory=False)
    tv = A.TwoViewCrop(16, 8, MEAN, STD, aug_view=True)
    a = tv(packed, torch.Generator().manual_seed(3))
    b = tv(packed, torch.Generator().manual_seed(3))
    assert set(a) == {'image', 'image4dalle', 'image_aug'}
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a['image'], a['image_aug'])          # an independent box
    assert set(A.TwoViewCrop(16, 8, MEAN, STD)(packed)) == {'image', 'image4dalle'}


# --------------------------------------------------------------------------------------------------------- refusals

def test_refusals():
    packed = A.pack_images([random_image(7, 5, 2)], pin_memory=False)
    tv = A.TwoViewCrop(16, 8, MEAN, STD)
    for box in [(0, 0, 8, 5), (0, 1, 7, 5), (-1, 0, 3, 3), (0, 0, 0, 3), (5, 3, 3, 3)]:
        with pytest.raises(ValueError, match='box|crop sides'):
            tv.apply(packed, [box], [False])
    with pytest.raises(ValueError, match='size'):
        A.TwoViewCrop(0, 8, MEAN, STD)
    with pytest.raises(ValueError, match='second_size'):
        A.TwoViewCrop(16, 1025, MEAN, STD)
    with pytest.raises(ValueError, match=r'uint8 \[H, W, 3\]'):
        A.pack_images([torch.zeros(4, 4, 4, dtype=torch.uint8)])
    with pytest.raises(ValueError, match=r'uint8 \[H, W, 3\]'):
        A.pack_images([torch.zeros(4, 4, 3)])
    with pytest.raises(ValueError, match='one box and one flip'):
        tv.apply(packed, [(0, 0, 7, 5)] * 2, [False] * 2)
    with pytest.raises(ValueError, match='not inside the packed buffer'):
        tv.apply({'pixels': packed['pixels'], 'table': ((0, 700, 5),)}, [(0, 0, 7, 5)], [False])
