"""augment.RandAugment on a CPU buffer: the torch restatement of DESIGN.md 4i against PIL (bit for bit), against the
reference's own table outputs (tests/golden/randaug_lut.npz, written by tools/gen_randaug_golden.py), exact geometric
identities, the plan sampler and the refusals.  tests/test_randaug_gpu.py compares the kernels with this restatement and
takes its packs from here.

Two packs of the same shapes.  (1, 1), (2, 5), (3, 3) have no interior or a one-pixel interior; (7, 5) has 35 pixels, so
Equalize's step is 0; (300, 230) has 69 000 pixels, channel 0 constant (one bin above 65 535, hi <= lo, step == 0),
channel 1 two-valued, channel 2 random.  The byte offsets 0, 3, 33, 60, 165, 9381, 47502 take every phase of a dword, and
rows of 5, 3, 131 and 230 pixels start on every phase too."""
import os

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageOps

from exploremultimodal_amd import augment as A
from exploremultimodal_amd import hip

SHAPES = [(1, 1), (2, 5), (3, 3), (7, 5), (64, 48), (97, 131), (300, 230)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'randaug_lut.npz')
OPS = {name: code for name, code in A.AUG_CODES.items()}


def random_pack():
    g = torch.Generator().manual_seed(77)
    ims = [torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8) for H, W in SHAPES]
    big = ims[-1]
    big[:, :, 0] = 201
    big[:, :, 1] = torch.where(torch.rand(300, 230, generator=g) < 0.3, 40, 180).to(torch.uint8)
    return ims


def pattern_pack():
    """Modular gradients and four-level images."""
    g = torch.Generator().manual_seed(78)
    ims = []
    for i, (H, W) in enumerate(SHAPES):
        if i % 2:
            ims.append((torch.randint(0, 4, (H, W, 3), generator=g) * 67 + 20).to(torch.uint8))
        else:
            y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
            ims.append(torch.stack([(3 * x + y) % 200 + 17, (x * y) % 97, (5 * y + 2 * x) % 256], dim=2).to(torch.uint8))
    return ims


@pytest.fixture(scope='module')
def packs():
    out = []
    for ims in (random_pack(), pattern_pack()):
        packed = A.pack_images(ims)
        assert [o for o, _, _ in packed['table']] == [0, 3, 33, 60, 165, 9381, 47502]       # every phase of a dword
        out.append((ims, packed))
    return out


def apply_one(packed, name, arg=0.0, fill=128):
    """Every image of the pack through one operation -> list of uint8 [H, W, 3] numpy arrays."""
    n = len(packed['table'])
    ra = A.RandAugment(n=1, augs=A.ALL_AUGS, fill=fill)
    plan = {'ops': torch.full((n, 1), OPS[name] if name else -1, dtype=torch.int64),
            'args': torch.full((n, 1), float(arg), dtype=torch.float64)}
    res = ra.apply(packed, plan)
    assert res['table'] is packed['table'] and res['pixels'].shape == packed['pixels'].shape
    return [A.unpack_image(res, i).numpy() for i in range(n)]


def _pil(im):
    return Image.fromarray(im.numpy())


def _count(name, got, want):
    bad = sum(int((g != np.asarray(w)).sum()) for g, w in zip(got, want))
    total = sum(g.size for g in got)
    print(f'{name}: {bad} of {total} values differ')
    return bad


# ------------------------------------------------------------------------------------------------ PIL, bit for bit

def test_autocontrast_equals_pil(packs):
    for ims, packed in packs:
        assert _count('AutoContrast', apply_one(packed, 'AutoContrast'), [ImageOps.autocontrast(_pil(im)) for im in ims]) == 0


def test_equalize_equals_pil(packs):
    for ims, packed in packs:
        assert _count('Equalize', apply_one(packed, 'Equalize'), [ImageOps.equalize(_pil(im)) for im in ims]) == 0


@pytest.mark.parametrize('factor', [0.28, 1.36])
def test_brightness_equals_pil(packs, factor):
    for ims, packed in packs:
        want = [ImageEnhance.Brightness(_pil(im)).enhance(factor) for im in ims]
        assert _count(f'Brightness {factor}', apply_one(packed, 'Brightness', factor), want) == 0


@pytest.mark.parametrize('factor', [0.28, 1.36, 1.9])
def test_sharpness_equals_pil(packs, factor):
    for ims, packed in packs:
        want = [ImageEnhance.Sharpness(_pil(im)).enhance(factor) for im in ims]
        assert _count(f'Sharpness {factor}', apply_one(packed, 'Sharpness', factor), want) == 0


def test_sharpness_one_is_the_identity(packs):
    ims, packed = packs[0]
    assert _count('Sharpness 1', apply_one(packed, 'Sharpness', 1.0), [im.numpy() for im in ims]) == 0


# ------------------------------------------------------------------------- the reference's own outputs, bit for bit

def test_table_operations_equal_the_reference():
    z = np.load(GOLDEN)
    n = int(z['n_images'])
    ims = [torch.from_numpy(z[f'in{i}']) for i in range(n)]
    packed = A.pack_images(ims)
    assert max(max(im.shape[:2]) for im in ims) <= 131
    assert _count('AutoContrast', apply_one(packed, 'AutoContrast'), [z[f'autocontrast{i}'] for i in range(n)]) == 0
    assert _count('Equalize', apply_one(packed, 'Equalize'), [z[f'equalize{i}'] for i in range(n)]) == 0
    assert sorted(z['levels'].tolist()) == [2, 7]
    for m in (7, 2):
        factor, thresh, bits = z[f'args_m{m}'].tolist()
        # the arguments the sampler would hand out are the reference's
        assert factor == A.aug_magnitude(hip.AUG_BRIGHTNESS, m) == A.aug_magnitude(hip.AUG_CONTRAST, m)
        assert thresh == A.aug_magnitude(hip.AUG_SOLARIZE, m) and bits == A.aug_magnitude(hip.AUG_POSTERIZE, m)
        for name, arg in (('Brightness', factor), ('Contrast', factor), ('Solarize', thresh), ('Posterize', bits)):
            want = [z[f'{name.lower()}{i}_m{m}'] for i in range(n)]
            assert _count(f'{name} m={m}', apply_one(packed, name, arg), want) == 0


def test_magnitudes_at_m7():
    mag = {name: A.aug_magnitude(code, 7) for name, code in A.AUG_CODES.items()}
    assert mag['Brightness'] == mag['Sharpness'] == mag['Contrast'] == 7 / 10 * 1.8 + 0.1
    assert abs(mag['Brightness'] - 1.36) < 1e-12 and abs(mag['ShearX'] - 0.21) < 1e-12 and mag['ShearX'] == mag['ShearY']
    assert mag['TranslateX'] == mag['TranslateY'] == 7.0 and mag['Rotate'] == 21.0
    assert mag['Solarize'] == 179.0 and mag['Posterize'] == 2.0
    assert mag['Identity'] == mag['AutoContrast'] == mag['Equalize'] == 0.0


# ------------------------------------------------------------------------------------------- geometric identities

@pytest.mark.parametrize('off', [3, -2, 7, -7])
def test_integer_translate_is_a_shift(packs, off):
    ims, packed = packs[0]
    for name, axis in (('TranslateX', 1), ('TranslateY', 0)):
        got = apply_one(packed, name, off)
        for g, im in zip(got, ims):
            im = im.numpy()
            want = np.full_like(im, 128)
            n = im.shape[axis]
            k = min(abs(off), n)
            # output position p samples source p + off
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            src[axis] = slice(k, n) if off > 0 else slice(0, n - k)
            dst[axis] = slice(0, n - k) if off > 0 else slice(k, n)
            want[tuple(dst)] = im[tuple(src)]
            assert np.array_equal(g, want), (name, off, im.shape)


def test_zero_shear_and_zero_rotation_are_the_identity(packs):
    for ims, packed in packs:
        for name in ('ShearX', 'ShearY', 'Rotate', 'TranslateX', 'TranslateY'):
            assert _count(f'{name} 0', apply_one(packed, name, 0.0), [im.numpy() for im in ims]) == 0


def test_unit_shear_shifts_the_rows(packs):
    ims, packed = packs[1]
    got = apply_one(packed, 'ShearX', 1.0, fill=9)
    for g, im in zip(got, ims):
        im = im.numpy()
        H, W, _ = im.shape
        want = np.full_like(im, 9)
        for y in range(H):                  # sx = x - y
            if y < W:
                want[y, y:] = im[y, :W - y]
        assert np.array_equal(g, want), im.shape


def test_slots_chain_and_skips_copy(packs):
    ims, packed = packs[0]
    n = len(ims)
    ra = A.RandAugment(n=2, augs=A.ALL_AUGS)
    plan = {'ops': torch.tensor([[OPS['TranslateX'], OPS['Equalize']]] * (n - 1) + [[-1, -1]]),
            'args': torch.tensor([[2.0, 0.0]] * n, dtype=torch.float64)}
    got = ra.apply(packed, plan)
    first = A.RandAugment(n=1, augs=A.ALL_AUGS).apply(packed, {'ops': plan['ops'][:, :1], 'args': plan['args'][:, :1]})
    second = A.RandAugment(n=1, augs=A.ALL_AUGS).apply(first, {'ops': plan['ops'][:, 1:], 'args': plan['args'][:, 1:]})
    assert torch.equal(got['pixels'], second['pixels'])
    assert torch.equal(A.unpack_image(got, n - 1), ims[-1])
    assert not torch.equal(got['pixels'], packed['pixels'])


# -------------------------------------------------------------------------------------------- plan and refusals

def test_plan_is_seeded():
    ra = A.RandAugment()
    a = ra.sample(500, torch.Generator().manual_seed(3))
    b = ra.sample(500, torch.Generator().manual_seed(3))
    c = ra.sample(500, torch.Generator().manual_seed(4))
    assert a['ops'].dtype == torch.int64 and a['args'].dtype == torch.float64
    assert tuple(a['ops'].shape) == tuple(a['args'].shape) == (500, 2) and not a['ops'].is_cuda
    assert torch.equal(a['ops'], b['ops']) and torch.equal(a['args'], b['args'])
    assert not torch.equal(a['ops'], c['ops'])


def test_plan_contents():
    augs = ('Equalize', 'ShearX', 'Rotate', 'Brightness')
    ra = A.RandAugment(n=3, m=7, augs=augs)
    plan = ra.sample(2000, torch.Generator().manual_seed(5))
    ops, args = plan['ops'], plan['args']
    codes = {OPS[a] for a in augs}
    assert set(ops.unique().tolist()) == codes | {-1}
    kept = (ops != -1).double().mean().item()
    assert abs(kept - 0.5) < 0.03                       # 6000 draws at p = 0.5: sigma = 0.0065
    for name in augs:
        mag = A.aug_magnitude(OPS[name], 7)
        vals = set(args[ops == OPS[name]].tolist())
        assert vals == ({mag, -mag} if name in ('ShearX', 'Rotate') else {mag}), (name, vals)
    assert (args[ops == -1] == 0).all()
    assert (A.RandAugment(prob=0.0).sample(300, torch.Generator().manual_seed(1))['ops'] == -1).all()
    assert (A.RandAugment(prob=1.0).sample(300, torch.Generator().manual_seed(1))['ops'] != -1).all()
    assert set(A.RandAugment(prob=1.0).sample(3000, torch.Generator().manual_seed(1))['ops'].unique().tolist()) == \
        {OPS[a] for a in A.PRETRAIN_AUGS}
    assert A.ALL_AUGS == A.PRETRAIN_AUGS + ('Solarize', 'Posterize', 'Contrast') and len(A.PRETRAIN_AUGS) == 10


def test_random_call_on_a_cpu_pack(packs):
    _, packed = packs[0]
    ra = A.RandAugment(prob=1.0)
    a = ra(packed, torch.Generator().manual_seed(11))
    b = ra(packed, torch.Generator().manual_seed(11))
    assert torch.equal(a['pixels'], b['pixels']) and a['table'] is packed['table']
    assert a['pixels'].dtype == torch.uint8 and a['pixels'].shape == packed['pixels'].shape
    assert not torch.equal(a['pixels'], packed['pixels'])


def test_refusals(packs):
    _, packed = packs[0]
    n = len(packed['table'])
    with pytest.raises(ValueError, match='unknown operation'):
        A.RandAugment(augs=('Identity', 'Cutout'))
    with pytest.raises(ValueError, match='Color'):
        A.RandAugment(augs=('Identity', 'Color'))
    for bad in (0, 5, 2.0):
        with pytest.raises(ValueError, match='n must be'):
            A.RandAugment(n=bad)
    ra = A.RandAugment(n=2, augs=A.ALL_AUGS)

    def plan(ops, args):
        return {'ops': torch.tensor(ops, dtype=torch.int64), 'args': torch.tensor(args, dtype=torch.float64)}

    with pytest.raises(ValueError, match='shape'):
        ra.apply(packed, plan([[0, 0]] * (n - 1), [[0.0, 0.0]] * (n - 1)))
    with pytest.raises(ValueError, match='shape'):
        ra.apply(packed, plan([[0]] * n, [[0.0]] * n))
    with pytest.raises(ValueError, match='shape'):
        ra.apply(packed, plan([[0, 0]] * n, [[0.0]] * n))
    for bits in (-1.0, 9.0, 2.5):
        with pytest.raises(ValueError, match='posterize'):
            ra.apply(packed, plan([[0, OPS['Posterize']]] * n, [[0.0, bits]] * n))
    for v in (float('nan'), float('inf')):
        with pytest.raises(ValueError, match='non-finite'):
            ra.apply(packed, plan([[OPS['Brightness'], 0]] * n, [[v, 0.0]] * n))
    with pytest.raises(ValueError, match='unknown op code'):
        ra.apply(packed, plan([[13, 0]] * n, [[0.0, 0.0]] * n))
    with pytest.raises(ValueError, match='contiguous 1-D uint8'):
        ra.apply({'pixels': packed['pixels'].float(), 'table': packed['table']}, plan([[0, 0]] * n, [[0.0, 0.0]] * n))
    with pytest.raises(ValueError, match='overlap'):
        ra.apply({'pixels': packed['pixels'], 'table': ((0, 2, 2), (3, 2, 2))}, plan([[0, 0]] * 2, [[0.0, 0.0]] * 2))
    with pytest.raises(ValueError, match='not inside'):
        ra.apply({'pixels': packed['pixels'][:16], 'table': ((0, 3, 2),)}, plan([[0, 0]], [[0.0, 0.0]]))
