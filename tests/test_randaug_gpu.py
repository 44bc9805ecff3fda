"""vlmo_randaug (csrc/randaug.hip) and the device path of augment.RandAugment against the CPU restatement of DESIGN.md 4i
(tests/test_randaug_cpu.py holds that restatement against PIL and the reference).

CASES is a list of two-slot plans.  Every case is applied to every image of both packs of test_randaug_cpu, and all of
it goes through ONE call of the entry point: the batch holds len(CASES) copies of the 14 images, the plan gives copy c the
slots of case c.  The arguments are those of m = 7 and m = 2 with both signs.

Bounds.  Table operations, Sharpness, copies, translates by an integer or a half (the bilinear value is then an integer or
an exact half in fp64, whatever is fused) and chains of those: the device bytes EQUAL the restatement's.  Shear, rotate
and other fractional offsets: the two sides may differ in fp64 contraction only, about 1e-13 in the interpolated value, so
a byte flips only where that value lies within 1e-13 of a rounding tie: at most 1 level, on at most 1 in 10 000 values of
the case (the 14 images of one case hold 509 004).  A tap-order or border error moves whole regions and fails this.
The library builds randaug.hip without contraction, and on an MI355X every case, these included, came out equal; built
with contraction, AutoContrast moved 48 310 values and Sharpness 1.36 moved 4 321, which the exact cases catch."""
import math

import numpy as np
import pytest
import torch

from exploremultimodal_amd import augment as A
from exploremultimodal_amd import hip
from tests import test_augment_cpu as crop_ref
from tests import test_randaug_cpu as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
O = ref.OPS
SKIP = ('', 0.0)
F7, F2 = A.aug_magnitude(hip.AUG_BRIGHTNESS, 7), A.aug_magnitude(hip.AUG_BRIGHTNESS, 2)      # 1.36, 0.46
S7, S2 = A.aug_magnitude(hip.AUG_SHEAR_X, 7), A.aug_magnitude(hip.AUG_SHEAR_X, 2)            # 0.21, 0.06
R7, R2 = A.aug_magnitude(hip.AUG_ROTATE, 7), A.aug_magnitude(hip.AUG_ROTATE, 2)              # 21, 6 degrees

# (slot 0, slot 1, exact): a slot is (name, argument), '' = skipped (-1)
EXACT_SINGLE = ([('Identity', 0.0), ('AutoContrast', 0.0), ('Equalize', 0.0), ('Solarize', 179.0), ('Solarize', 51.0),
                 ('Posterize', 2.0), ('Posterize', 0.0), ('Posterize', 8.0)]
                + [(name, f) for name in ('Brightness', 'Sharpness', 'Contrast') for f in (F7, F2)]
                + [('Sharpness', 1.9), ('Sharpness', 1.0)]
                + [(name, off) for name in ('TranslateX', 'TranslateY') for off in (7.0, -7.0, 2.0, -2.0, 2.5, 400.0)])
NEAR_SINGLE = ([(name, s) for name in ('ShearX', 'ShearY') for s in (S7, -S7, S2, -S2)]
               + [('Rotate', r) for r in (R7, -R7, R2, -R2, 90.0)] + [('TranslateX', 2.3), ('TranslateY', -0.7)])
CASES = ([(op, SKIP, True) for op in EXACT_SINGLE] + [(SKIP, op, False) for op in NEAR_SINGLE]
         + [(SKIP, SKIP, True), (SKIP, ('Brightness', F7), True), (('Identity', 0.0), ('Equalize', 0.0), True),
            # a statistics op after a warp, a filter after a warp: the second slot must read what the first wrote
            (('TranslateX', 2.5), ('Equalize', 0.0), True), (('TranslateY', -7.0), ('AutoContrast', 0.0), True),
            (('TranslateX', -2.0), ('Contrast', F7), True), (('TranslateY', 2.5), ('Sharpness', F7), True),
            (('Equalize', 0.0), ('Sharpness', F2), True), (('AutoContrast', 0.0), ('Equalize', 0.0), True),
            # a warp after a sharpen
            (('Sharpness', F7), ('Rotate', R7), False), (('Sharpness', 1.9), ('ShearY', -S7), False),
            (('Sharpness', F7), ('TranslateX', 7.0), True)])


def _plan(cases, per_case):
    ops = [[O[name] if name else -1 for name, _ in (a, b)] for a, b, _ in cases for _ in range(per_case)]
    args = [[arg for _, arg in (a, b)] for a, b, _ in cases for _ in range(per_case)]
    return {'ops': torch.tensor(ops, dtype=torch.int64), 'args': torch.tensor(args, dtype=torch.float64)}


@pytest.fixture(scope='module')
def batch():
    ims = ref.random_pack() + ref.pattern_pack()
    packed = A.pack_images(ims * len(CASES))
    plan = _plan(CASES, len(ims))
    ra = A.RandAugment(n=2, augs=A.ALL_AUGS)
    want = ra.apply(packed, plan)
    dev = {'pixels': packed['pixels'].to(DEV), 'table': packed['table']}
    got = ra.apply(dev, plan)
    torch.cuda.synchronize()
    assert got['pixels'].is_cuda and got['pixels'].dtype == torch.uint8 and got['table'] is packed['table']
    return ims, packed, dev, plan, ra, want, {'pixels': got['pixels'].cpu(), 'table': got['table']}


def test_every_case_against_the_restatement(batch):
    ims, packed, _, _, _, want, got = batch
    k = len(ims)
    report = []
    for c, case in enumerate(CASES):
        diff = np.concatenate([(A.unpack_image(got, c * k + i).numpy().astype(np.int16)
                                - A.unpack_image(want, c * k + i).numpy().astype(np.int16)).reshape(-1) for i in range(k)])
        report.append((case, int((diff != 0).sum()), int(np.abs(diff).max()), diff.size))
        print(f'{case}: {report[-1][1]} of {diff.size} values differ, by at most {report[-1][2]}')
    for case, n_bad, worst, size in report:
        if case[2]:
            assert n_bad == 0, case
        else:
            assert worst <= 1 and n_bad <= size // 10000, case
    # the padding behind the last image is zero, as pack_images leaves it
    end = packed['table'][-1][0] + 300 * 230 * 3
    assert not got['pixels'][end:].any()
    # and the cases did something: every case but the copies changed the batch
    for c, case in enumerate(CASES):
        same = all(torch.equal(A.unpack_image(got, c * k + i), ims[i]) for i in range(k))
        copies = all(name in ('', 'Identity') or (name, arg) in (('Posterize', 8.0), ('Sharpness', 1.0))
                     for name, arg in case[:2])
        assert same == copies, case


def test_second_call_is_bit_identical(batch):
    _, _, dev, plan, ra, _, got = batch
    again = ra.apply(dev, plan)['pixels'].cpu()
    assert torch.equal(again, got['pixels'])


def test_image_order_does_not_matter(batch):
    ims, packed, _, plan, ra, _, got = batch
    n = len(packed['table'])
    rev = A.pack_images(list(reversed(ims * len(CASES))))
    rplan = {'ops': plan['ops'].flip(0), 'args': plan['args'].flip(0)}
    out = ra.apply({'pixels': rev['pixels'].to(DEV), 'table': rev['table']}, rplan)
    out = {'pixels': out['pixels'].cpu(), 'table': out['table']}
    for i in range(n):
        assert torch.equal(A.unpack_image(out, n - 1 - i), A.unpack_image(got, i)), (i, CASES[i // len(ims)])


def test_one_and_four_slots():
    ims = ref.random_pack()
    packed = A.pack_images(ims)
    dev = {'pixels': packed['pixels'].to(DEV), 'table': packed['table']}
    n = len(ims)
    for slots in ([('Equalize', 0.0)],
                  [('Sharpness', F7), ('TranslateX', -7.0), ('AutoContrast', 0.0), ('Solarize', 179.0)],
                  [('TranslateY', 2.5), ('Contrast', F2), ('Sharpness', F2)]):
        ra = A.RandAugment(n=len(slots), augs=A.ALL_AUGS)
        plan = {'ops': torch.tensor([[O[name] for name, _ in slots]] * n),
                'args': torch.tensor([[arg for _, arg in slots]] * n, dtype=torch.float64)}
        assert torch.equal(ra.apply(dev, plan)['pixels'].cpu(), ra.apply(packed, plan)['pixels']), slots


def test_random_call_feeds_the_crop():
    """ra in front of tv on the device against the same on the CPU buffer, with a plan of exact operations only."""
    ims = ref.random_pack()[3:] + ref.pattern_pack()[3:]
    packed = A.pack_images(ims)
    dev = {'pixels': packed['pixels'].to(DEV), 'table': packed['table']}
    slots = [(('Equalize', 0.0), ('Sharpness', F7)), (('TranslateX', 7.0), ('AutoContrast', 0.0)),
             (('Brightness', F7), SKIP), (SKIP, SKIP), (('Sharpness', F2), ('TranslateY', -7.0)),
             (('Contrast', F7), ('Solarize', 179.0)), (('Identity', 0.0), ('Posterize', 2.0)), (('Equalize', 0.0), SKIP)]
    plan = _plan([(a, b, True) for a, b in slots], 1)
    ra = A.RandAugment(n=2, augs=A.ALL_AUGS)
    tv = A.TwoViewCrop(16, 8, crop_ref.MEAN, crop_ref.STD)
    boxes = [(0, 0, H, W) if i % 2 else (H // 4, W // 5, H // 2, W // 2) for i, (H, W, _) in enumerate(im.shape for im in ims)]
    flips = [bool(i % 3 == 0) for i in range(len(ims))]
    got = tv.apply(ra.apply(dev, plan), boxes, flips)
    want = tv.apply(ra.apply(packed, plan), boxes, flips)
    for name, tol in (('image', crop_ref.ATOL), ('image4dalle', 0.8 * crop_ref.PIXEL_TOL)):
        err = (got[name].cpu().double() - want[name].double()).abs().max().item()
        print(f'{name}: max |device - cpu| = {err:.3g} (bound {tol:.3g})')
        assert got[name].is_cuda and err <= tol
    both = tv(A.RandAugment()(dev, torch.Generator().manual_seed(5)), torch.Generator().manual_seed(6))
    assert all(torch.isfinite(v).all() for v in both.values())


def test_entry_point_refusals():
    ims = ref.random_pack()
    packed = A.pack_images(ims)
    pixels, table = packed['pixels'].to(DEV), packed['table']
    n = len(table)
    zeros = [[0.0]] * n

    def call(pixels=pixels, table=table, ops=[[hip.AUG_EQUALIZE]] * n, a=zeros, b=zeros, **kw):
        return hip.randaug(pixels, table, ops, a, b, **kw)

    call()
    with pytest.raises(RuntimeError, match='vlmo_randaug.*4-byte'):
        call(pixels=pixels[1:-3], table=((0, 1, 1),), ops=[[0]], a=[[0.0]], b=[[0.0]])
    with pytest.raises(RuntimeError, match='vlmo_randaug.*workspace'):
        call(ws=torch.empty(n * 3840 // 4 - 1, dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError, match='vlmo_randaug.*slots'):
        call(ops=[[0] * 5] * n, a=[[0.0] * 5] * n, b=[[0.0] * 5] * n)
    with pytest.raises(RuntimeError, match='vlmo_randaug.*unknown op'):
        call(ops=[[13]] * n)
    with pytest.raises(RuntimeError, match='vlmo_randaug.*posterize'):
        call(ops=[[hip.AUG_POSTERIZE]] * n, a=[[9.0]] * n)
    with pytest.raises(RuntimeError, match='vlmo_randaug.*non-finite'):
        call(ops=[[hip.AUG_BRIGHTNESS]] * n, a=[[math.inf]] * n)
    with pytest.raises(RuntimeError, match='vlmo_randaug.*overlap'):
        call(table=((0, 2, 2), (3, 2, 2)), ops=[[0]] * 2, a=[[0.0]] * 2, b=[[0.0]] * 2)
    with pytest.raises(RuntimeError, match='vlmo_randaug.*not inside'):
        call(table=((pixels.numel() - 2, 1, 1),), ops=[[0]], a=[[0.0]], b=[[0.0]])
    with pytest.raises(RuntimeError, match='vlmo_randaug.*must not overlap'):
        call(out=pixels)
    torch.cuda.synchronize()
