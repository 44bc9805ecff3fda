"""vlmo_crop_resample (csrc/augment.hip) and the device path of augment.TwoViewCrop against the fp64 restatement of the
definition in tests/test_augment_cpu.py.

One pack of five images, (H, W) = (1, 1), (7, 5), (64, 48), (97, 131), (300, 200): their byte offsets are 0, 3, 108, 9324
and 47445, so images and rows start on odd bytes.  Every case of JOBS goes through ONE call of the entry point (two
launches); TwoViewCrop has one output size per view, so the list is handed to hip.crop_resample, the call
TwoViewCrop.apply makes, and apply itself is checked on the same pack further down.

Tolerance (derived, not measured; see tests/test_augment_cpu.py): 2e-5 on pixel values in [0, 1], i.e. atol = 2e-5 /
min(std) on the normalised outputs and 0.8 * 2e-5 after map_pixels, rtol = 0."""
from functools import partial

import numpy as np
import pytest
import torch

from exploremultimodal_amd import augment as A
from exploremultimodal_amd import hip
from exploremultimodal_amd.dvae import logit_laplace_eps
from oracle import synth
from tests import test_augment_cpu as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MEAN, STD = ref.MEAN, ref.STD
BIC, LAN = hip.FILTER_BICUBIC, hip.FILTER_LANCZOS
NORM, DALLE = hip.FINISH_NORMALIZE, hip.FINISH_MAP_PIXELS
TOL = {NORM: ref.ATOL, DALLE: 0.8 * ref.PIXEL_TOL}
SHAPES = [(1, 1), (7, 5), (64, 48), (97, 131), (300, 200)]

# (image, (top, left, h, w), flip, S, filter, finish)
JOBS = [
    (3, (20, 30, 37, 53), 0, 16, BIC, NORM),        # non-integer downscale, h != w
    (3, (20, 30, 37, 53), 0, 8, LAN, DALLE),
    (3, (20, 30, 37, 53), 1, 16, BIC, NORM),        # the same box mirrored
    (3, (20, 30, 37, 53), 1, 8, LAN, DALLE),
    (2, (3, 4, 5, 7), 0, 16, BIC, NORM),            # upscale
    (2, (3, 4, 5, 7), 1, 16, LAN, DALLE),
    (1, (0, 0, 7, 5), 0, 17, BIC, NORM),            # whole images
    (2, (0, 0, 64, 48), 1, 224, BIC, NORM),
    (3, (0, 0, 97, 131), 0, 17, LAN, DALLE),
    (3, (0, 0, 40, 50), 0, 16, BIC, NORM),          # boxes touching each border
    (3, (57, 81, 40, 50), 1, 17, BIC, DALLE),
    (3, (57, 0, 40, 50), 0, 17, LAN, NORM),
    (3, (0, 81, 40, 50), 1, 16, LAN, DALLE),
    (0, (0, 0, 1, 1), 0, 16, BIC, NORM),            # 1 x 1 boxes: the first and the last pixel of the buffer
    (4, (299, 199, 1, 1), 1, 17, LAN, DALLE),
    (4, (10, 7, 280, 190), 1, 224, BIC, NORM),      # 224 wide: 3.5 tiles of 64 columns, 7 of 32
    (4, (10, 7, 280, 190), 0, 224, LAN, DALLE),
    (4, (0, 0, 300, 200), 0, 8, LAN, DALLE),        # the largest downscale: 225 vertical taps, two chunks
    (4, (0, 0, 300, 200), 1, 8, LAN, NORM),
    (4, (0, 0, 300, 200), 0, 8, BIC, NORM),
]


@pytest.fixture(scope='module')
def pack():
    ims = [ref.random_image(H, W, 40 + i) for i, (H, W) in enumerate(SHAPES)]
    packed = A.pack_images(ims)
    assert [o for o, _, _ in packed['table']] == [0, 3, 108, 9324, 47445]
    dev = {'pixels': packed['pixels'].to(DEV), 'table': packed['table']}
    return ims, packed, dev


def _run(dev, jobs):
    outs = [torch.full((3, S, S), float('nan'), device=DEV) for _, _, _, S, _, _ in jobs]
    hip.crop_resample(dev['pixels'], dev['table'],
                      [(im,) + box + (flip, S, filt, fin, out) for (im, box, flip, S, filt, fin), out in zip(jobs, outs)],
                      MEAN, STD, logit_laplace_eps)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


@pytest.fixture(scope='module')
def results(pack):
    ims, _, dev = pack
    got = _run(dev, JOBS)
    want = [ref.view(ims[im].numpy(), box, flip, S, filt, 'norm' if fin == NORM else 'dalle')
            for im, box, flip, S, filt, fin in JOBS]
    return got, want


def test_every_case_against_the_restatement(results):
    got, want = results
    worst = 0.0
    for job, g, w in zip(JOBS, got, want):
        assert torch.isfinite(g).all(), job
        err = np.abs(g.double().numpy() - w).max()
        worst = max(worst, err / TOL[job[5]])
        print(f'{job}: max |hip - fp64| = {err:.3g} (bound {TOL[job[5]]:.3g})')
    print(f'largest error / bound = {worst:.3g}')
    for job, g, w in zip(JOBS, got, want):
        assert np.abs(g.double().numpy() - w).max() <= TOL[job[5]], job


def test_second_call_is_bit_identical(pack, results):
    again = _run(pack[2], JOBS)
    assert all(torch.equal(a, b) for a, b in zip(again, results[0]))


def test_job_order_does_not_matter(pack, results):
    order = torch.randperm(len(JOBS), generator=torch.Generator().manual_seed(2)).tolist()
    assert order != sorted(order)
    shuffled = _run(pack[2], [JOBS[i] for i in order])
    for pos, i in enumerate(order):
        assert torch.equal(shuffled[pos], results[0][i]), JOBS[i]


def test_apply_on_the_device(pack):
    ims, packed, dev = pack
    tv = A.TwoViewCrop(16, 8, MEAN, STD, aug_view=True)
    boxes = [(0, 0, 1, 1), (1, 0, 5, 5), (10, 3, 37, 30), (20, 30, 37, 53), (0, 0, 300, 200)]
    flips = [True, False, True, False, True]
    aug_boxes = [(0, 0, 1, 1), (0, 0, 7, 5), (27, 18, 37, 30), (44, 78, 53, 53), (150, 100, 150, 100)]
    aug_flips = [False, True, False, True, False]
    got = tv.apply(dev, boxes, flips, aug_boxes, aug_flips)
    want = ref.reference_views([im.numpy() for im in ims], tv, boxes, flips, aug_boxes, aug_flips)
    assert set(got) == {'image', 'image4dalle', 'image_aug'}
    for name, tol in (('image', TOL[NORM]), ('image_aug', TOL[NORM]), ('image4dalle', TOL[DALLE])):
        assert got[name].is_cuda and got[name].dtype == torch.float32 and tuple(got[name].shape) == want[name].shape
        err = np.abs(got[name].double().cpu().numpy() - want[name]).max()
        print(f'{name}: max |hip - fp64| = {err:.3g} (bound {tol:.3g})')
        assert err <= tol
    two = A.TwoViewCrop(16, 8, MEAN, STD)(dev, torch.Generator().manual_seed(1))
    assert set(two) == {'image', 'image4dalle'} and all(torch.isfinite(v).all() for v in two.values())


def test_views_feed_the_backbone_and_the_dvae(pack):
    """image -> VLMO.forward_features, image4dalle -> Dalle_VAE.get_codebook_indices, at the dtypes and layouts the crop
    writes, for the synthetic mini configuration (64 px, dVAE at 32 px)."""
    from exploremultimodal_amd.dvae import create_d_vae
    from exploremultimodal_amd.vlmo import VLMO, LayerNorm
    _, _, dev = pack
    mc = synth.make_config('mini').model
    sd = synth.synth_backbone_state_dict(mc, 0, [('v', 'l', 'vl')] * mc.depth)
    model = VLMO(img_size=mc.img_size, patch_size=mc.patch_size, embed_dim=mc.embed_dim, depth=mc.depth,
                 num_heads=mc.num_heads, mlp_ratio=mc.mlp_ratio, qkv_bias=True, norm_layer=partial(LayerNorm, eps=1e-12),
                 init_values=mc.init_values, vocab_size=mc.vocab_size, max_text_len=mc.max_text_len,
                 fusion_layer=mc.fusion_layer)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    B = len(SHAPES)
    tv = A.TwoViewCrop(mc.img_size, mc.img_size // 2, MEAN, STD, aug_view=True)
    views = tv(dev, torch.Generator().manual_seed(9))
    assert tuple(views['image'].shape) == (B, 3, mc.img_size, mc.img_size)
    assert tuple(views['image4dalle'].shape) == (B, 3, mc.img_size // 2, mc.img_size // 2)
    batch = synth.synth_batch(mc, B)
    mask = torch.ones(B, synth.num_img_tokens(mc), dtype=torch.int64, device=DEV)
    with torch.no_grad():
        for key in ('image', 'image_aug'):
            x, _ = model.forward_features(img=views[key], txt=batch['text_ids'].to(DEV), img_attn_masks=mask,
                                          txt_attn_masks=batch['text_mask'].to(DEV))
            assert torch.isfinite(x.float()).all()
        vae = create_d_vae(None, 'dall-e', mc.img_size // 2, DEV, vocab_size=1024)
        ids = vae.get_codebook_indices(views['image4dalle'])
    g = mc.img_size // 16
    assert tuple(ids.shape) == (B, g, g) and ids.dtype == torch.int64 and 0 <= ids.min().item() <= ids.max().item() < 1024


def test_refusals(pack):
    _, _, dev = pack
    tv = A.TwoViewCrop(16, 8, MEAN, STD)
    with pytest.raises(ValueError, match='not inside'):
        tv.apply(dev, [(0, 0, 2, 1)] + [(0, 0, 1, 1)] * 4, [False] * 5)
    out = torch.empty(3, 16, 16, device=DEV)
    for job, msg in (((4, 0, 0, 301, 200, 0, 16, BIC, NORM, out), 'not inside'),
                     ((4, 0, 1, 300, 200, 0, 16, BIC, NORM, out), 'not inside'),
                     ((5, 0, 0, 1, 1, 0, 16, BIC, NORM, out), 'image index'),
                     ((4, 0, 0, 1, 1, 0, 16, 2, NORM, out), 'filter')):
        with pytest.raises(RuntimeError, match=msg):
            hip.crop_resample(dev['pixels'], dev['table'], [job], MEAN, STD, logit_laplace_eps)
    for S in (0, 1025):
        with pytest.raises(RuntimeError, match='S <= 1024'):
            hip.crop_resample(dev['pixels'], dev['table'], [(4, 0, 0, 1, 1, 0, S, BIC, NORM, torch.empty(3, S, S, device=DEV))],
                              MEAN, STD, logit_laplace_eps)
    with pytest.raises(RuntimeError, match='4-byte'):
        hip.crop_resample(dev['pixels'][1:], ((0, 1, 1),), [(0, 0, 0, 1, 1, 0, 16, BIC, NORM, out)], MEAN, STD,
                          logit_laplace_eps)
    torch.cuda.synchronize()
