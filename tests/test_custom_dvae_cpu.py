"""BEiT's DiscreteVAE (discrete_vae_type = 'customized') without a GPU: state-dict keys against the reference class's
(tests/golden/custom_dvae_keys.json, written by tools/gen_custom_dvae_golden.py), construction, the refused shapes, and
the engine's weight layouts against torch: the index maps of vlmo_conv4s2_nhwc / vlmo_convt4s2_nhwc / vlmo_dvae_patch4s2
(include/vlmo_hip.h) restated with torch gathers on the CPU and applied to the shadow weights must give
F.conv2d(stride=2, padding=1) / F.conv_transpose2d(stride=2, padding=1)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from exploremultimodal_amd import dvae, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = {
    'custom_dvae_small': dict(image_size=32, num_tokens=512, codebook_dim=64, num_layers=3, hidden_dim=64),
    'custom_dvae_full_b2': dict(image_size=112, num_tokens=8192, codebook_dim=512, num_layers=3, hidden_dim=256),
}


def _dims(case):
    return {k: v for k, v in CASES[case].items() if k != 'image_size'}


@pytest.mark.parametrize('case', list(CASES))
def test_state_dict_keys_match_reference(case):
    want = json.load(open(os.path.join(GOLDEN, 'custom_dvae_keys.json')))[case]
    vae = dvae.DiscreteVAE(**CASES[case])
    got = {k: list(v.shape) for k, v in vae.state_dict().items()}
    assert got == want
    sd = synth.synth_custom_dvae_state_dict(0, **_dims(case))
    assert {k: list(v.shape) for k, v in sd.items()} == want
    vae.load_state_dict(sd, strict=True)


def test_fixture_contents():
    for case, dims in CASES.items():
        g = np.load(os.path.join(GOLDEN, case + '.npz'))
        s, n = dims['image_size'], dims['image_size'] // 8
        assert g['image16'].shape == (2, 3, s, s) and g['image16'].dtype == np.float16
        assert g['ids'].shape == (2, n, n) and g['ids'].dtype == np.int64
        assert 0 <= g['ids'].min() and g['ids'].max() < dims['num_tokens']
        assert g['top2_gap'].shape == (2, n, n) and (g['top2_gap'] >= 0).all()
        assert g['decoded'].shape == (2, 3, s, s)
        assert 0 < float(g['sim_err_logits']) < 0.1 and 0 < float(g['sim_err_decoded']) < 0.1
        # what the generator asserted on the reference
        assert (g['top2_gap'] < 8 * float(g['sim_err_logits'])).mean() <= 0.20
        if 'logits' in g.files:
            assert np.array_equal(g['logits'].argmax(1), g['ids'])
        else:
            flat_ids = g['ids'].reshape(-1)
            assert np.array_equal(g['logits_sample'].argmax(1), flat_ids[g['logit_rows']])
    assert len(np.unique(np.load(os.path.join(GOLDEN, 'custom_dvae_full_b2.npz'))['ids'])) >= 392 // 4


def test_create_d_vae_customized_random_init():
    vae = dvae.create_d_vae(None, 'customized', 32, 'cpu', vocab_size=512)
    assert isinstance(vae, dvae.DiscreteVAE)
    assert (vae.num_tokens, vae.num_layers, vae.codebook_dim, vae.hidden_dim) == (512, 3, 512, 256)
    assert vae.get_image_size() == 32 and vae.get_image_tokens_size() == 4
    # without weights AND without a vocabulary there is nothing to build: refused, with a message that says what to pass
    with pytest.raises(NotImplementedError, match='vocab_size'):
        dvae.create_d_vae(None, 'customized', 32, 'cpu')
    # the dall-e branch is what it was (8192 tokens by default)
    assert dvae.create_d_vae(None, 'dall-e', 32, 'cpu').encoder.vocab_size == 8192
    assert isinstance(dvae.create_d_vae(None, 'dall-e', 32, 'cpu', vocab_size=512), dvae.Dalle_VAE)


def test_create_d_vae_customized_loads_reference_checkpoint(tmp_path):
    """<path>/pytorch_model.bin['weights'] as get_d_vae reads it (objectives.py:610-628)."""
    sd = synth.synth_custom_dvae_state_dict(0)
    torch.save({'weights': sd}, tmp_path / 'pytorch_model.bin')
    vae = dvae.create_d_vae(str(tmp_path), 'customized', 112, 'cpu')
    assert (vae.num_tokens, vae.codebook_dim, vae.hidden_dim, vae.image_size) == (8192, 512, 256, 112)
    got = vae.state_dict()
    assert list(got) == list(sd)
    for k in sd:
        assert torch.equal(got[k], sd[k]), k


def test_unknown_type_raises_with_message():
    with pytest.raises(NotImplementedError, match="'dall-e', 'customized'"):
        dvae.create_d_vae(None, 'vqgan', 32, 'cpu')


@pytest.mark.parametrize('over, match', [
    (dict(hidden_dim=96), 'hidden_dim'),
    (dict(hidden_dim=32), 'hidden_dim'),
    (dict(num_tokens=1000), 'num_tokens'),
    (dict(codebook_dim=20), 'codebook_dim'),
    (dict(channels=1), 'channels'),
    (dict(image_size=36), 'image_size'),
    (dict(image_size=4, num_layers=3), 'image_size'),
])
def test_limits_refuse(over, match):
    kw = dict(CASES['custom_dvae_small'])
    kw.update(over)
    with pytest.raises(NotImplementedError, match=match):
        dvae.DiscreteVAE(**kw)
    with pytest.raises(ValueError, match='layers'):
        dvae.DiscreteVAE(num_layers=0)


def test_training_pass_and_cpu_tensors_refused():
    vae = dvae.DiscreteVAE(**CASES['custom_dvae_small'])
    img = torch.zeros(1, 3, 32, 32)
    with pytest.raises(NotImplementedError, match='Gumbel-softmax training pass'):
        vae(img)
    with pytest.raises(RuntimeError, match='cuda'):
        vae.get_codebook_indices(img)
    with pytest.raises(RuntimeError, match='cuda'):
        vae.decode(torch.zeros(1, 16, dtype=torch.int64))
    with pytest.raises(ValueError, match='image size'):
        vae.get_codebook_indices(torch.zeros(1, 3, 16, 16))


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' index maps, restated with torch on NHWC tensors

def _shifted(x, dy, dx, stride, Ho, Wo):
    """x [B, H, W, C] -> [B, Ho, Wo, C]: pixel (stride * oy + dy, stride * ox + dx), zero outside the image."""
    B, H, W, C = x.shape
    oy = stride * torch.arange(Ho) + dy
    ox = stride * torch.arange(Wo) + dx
    ok = ((oy >= 0) & (oy < H))[:, None] & ((ox >= 0) & (ox < W))[None, :]
    g = x[:, oy.clamp(0, H - 1)][:, :, ox.clamp(0, W - 1)]
    return g * ok[None, :, :, None].to(x.dtype)


def conv4s2_by_index_map(x, shadow):
    """vlmo_conv4s2_nhwc: output (oy, ox) reads input (2 oy - 1 + ky, 2 ox - 1 + kx) against columns
    [(4 ky + kx) * Cin, + Cin) of shadow [Cout, 16 * Cin]."""
    B, H, W, C = x.shape
    out = torch.zeros(B, H // 2, W // 2, shadow.shape[0], dtype=x.dtype)
    for t in range(16):
        ky, kx = t // 4, t % 4
        out += _shifted(x, ky - 1, kx - 1, 2, H // 2, W // 2) @ shadow[:, t * C:(t + 1) * C].t()
    return out


def convT4s2_by_index_map(x, shadow):
    """vlmo_convt4s2_nhwc: output (2 y + py, 2 x + px) sums input (y + py - a, x + px - b) against columns
    [(2 a + b) * Cin, + Cin) of quarter 2 py + px of shadow [4, Cout, 4 * Cin]."""
    B, H, W, C = x.shape
    out = torch.full((B, 2 * H, 2 * W, shadow.shape[1]), float('nan'), dtype=x.dtype)
    for p in range(4):
        py, px = p // 2, p % 2
        acc = torch.zeros(B, H, W, shadow.shape[1], dtype=x.dtype)
        for t in range(4):
            a, b = t // 2, t % 2
            acc += _shifted(x, py - a, px - b, 1, H, W) @ shadow[p][:, t * C:(t + 1) * C].t()
        out[:, py::2, px::2] = acc
    return out


def patch4s2_by_index_map(img, kpad):
    """vlmo_dvae_patch4s2: column c * 16 + ky * 4 + kx of row (b, oy, ox) = img[b, c, 2 oy - 1 + ky, 2 ox - 1 + kx]."""
    B, C, H, W = img.shape
    x = img.permute(0, 2, 3, 1)
    cols = torch.zeros(B, H // 2, W // 2, kpad, dtype=img.dtype)
    for c in range(C):
        for ky in range(4):
            for kx in range(4):
                cols[..., c * 16 + ky * 4 + kx] = _shifted(x[..., c:c + 1], ky - 1, kx - 1, 2, H // 2, W // 2)[..., 0]
    return cols


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).double()


@pytest.mark.parametrize('B, H, W, Cin, Cout', [(2, 6, 10, 8, 5), (1, 2, 2, 4, 3)])
def test_conv4s2_shadow_layout(B, H, W, Cin, Cout):
    x, w = _ints((B, Cin, H, W), -3, 4, 1), _ints((Cout, Cin, 4, 4), -2, 3, 2)
    want = F.conv2d(x, w, stride=2, padding=1).permute(0, 2, 3, 1)
    shadow = dvae.tap_major_shadow(w)
    assert shadow.dtype == torch.float16 and shadow.shape == (Cout, 16 * Cin)
    got = conv4s2_by_index_map(x.permute(0, 2, 3, 1), shadow.double())
    assert torch.equal(got, want)


@pytest.mark.parametrize('B, H, W, Cin, Cout, pad', [(2, 3, 5, 8, 6, None), (1, 1, 1, 4, 3, None), (1, 2, 3, 8, 4, 64)])
def test_convT4s2_shadow_layout(B, H, W, Cin, Cout, pad):
    x, w = _ints((B, Cin, H, W), -3, 4, 3), _ints((Cin, Cout, 4, 4), -2, 3, 4)
    want = F.conv_transpose2d(x, w, stride=2, padding=1).permute(0, 2, 3, 1)
    shadow = dvae.convT4s2_shadow(w, pad)
    cp = pad or Cin
    assert shadow.dtype == torch.float16 and shadow.shape == (4, Cout, 4 * cp)
    xn = F.pad(x.permute(0, 2, 3, 1), (0, cp - Cin))
    got = convT4s2_by_index_map(xn, shadow.double())
    assert not torch.isnan(got).any(), 'the four parities do not cover the output'
    assert torch.equal(got, want)
    if (H, W) == (1, 1):        # one input pixel: the output is the centre 2 x 2 of the kernel
        assert torch.equal(got[0].permute(2, 0, 1), (x[0, :, 0, 0, None, None, None] * w[:, :, 1:3, 1:3]).sum(0))


def test_stem_patch_layout():
    img, w = _ints((2, 3, 8, 12), -4, 5, 5), _ints((7, 3, 4, 4), -2, 3, 6)
    cols = patch4s2_by_index_map(img, 64)
    assert (cols[..., 48:] == 0).all()
    ws = F.pad(w.reshape(7, -1), (0, 16))        # the stem shadow of DiscreteVAE._features: (c, ky, kx) order, K 48 -> 64
    assert torch.equal(cols @ ws.t(), F.conv2d(img, w, stride=2, padding=1).permute(0, 2, 3, 1))
