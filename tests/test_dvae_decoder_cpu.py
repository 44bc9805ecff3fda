"""Host side of the dVAE decoder (exploremultimodal_amd/dvae.py: DecoderBlock, Decoder, Dalle_VAE.decode / forward,
unmap_pixels) against fixtures made from the reference (tools/gen_decoder_golden.py).  No GPU: module layout, state-dict
keys, the fixture itself, pickle loading and the wrapper's behaviour without a decoder."""
import json
import os
import shutil
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from exploremultimodal_amd import dvae, synth

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
ENC_PKL = os.path.join(GOLDEN, 'dvae_encoder_pickle.pkl')
SMALL = dict(n_hid=256, vocab_size=1024)


@pytest.mark.parametrize('name,kw', [('default', {}), ('n_hid=256,vocab_size=1024', SMALL)])
def test_state_dict_keys_and_shapes_equal_the_reference(name, kw):
    ref = json.load(open(os.path.join(GOLDEN, 'dvae_dec_keys.json')))[name]
    ours = {k: list(v.shape) for k, v in dvae.Decoder(**kw).state_dict().items()}
    assert ours == ref
    # the synthetic recipe addresses exactly these tensors
    sd = synth.synth_dvae_decoder_state_dict(0, **kw)
    assert {k: list(v.shape) for k, v in sd.items()} == ref


def _restated(dec, z):
    """dall_e/decoder.py:45-46, 75-124 written out with F.conv2d / F.interpolate over the mirror's parameters."""
    conv = lambda m, x: F.conv2d(x, m.w, m.b, padding=(m.kw - 1) // 2)
    x = conv(dec.blocks.input, z)
    for g in range(1, 5):
        grp = getattr(dec.blocks, f'group_{g}')
        for bi in range(1, dec.n_blk_per_group + 1):
            blk = getattr(grp, f'block_{bi}')
            t = x
            for ci in (1, 2, 3, 4):
                t = conv(getattr(blk.res_path, f'conv_{ci}'), t.relu())
            idp = conv(blk.id_path, x) if isinstance(blk.id_path, dvae.Conv2d) else x
            x = idp + blk.post_gain * t
        if g < 4:
            x = F.interpolate(x, scale_factor=2, mode='nearest')
    return conv(dec.blocks.output.conv, x.relu())


def test_restated_decoder_reproduces_the_small_fixture():
    g = np.load(os.path.join(GOLDEN, 'dvae_dec_small.npz'))
    dec = dvae.Decoder(**SMALL)
    dec.load_state_dict(synth.synth_dvae_decoder_state_dict(0, **SMALL), strict=True)
    ids = torch.from_numpy(g['ids'])
    assert ids.shape == (2, 4, 4) and ids.dtype == torch.int64
    z = F.one_hot(ids, num_classes=1024).permute(0, 3, 1, 2).float()
    with torch.no_grad():
        y = _restated(dec, z)
    ref = torch.from_numpy(g['y'])
    assert y.shape == ref.shape == (2, 6, 32, 32)
    assert (y - ref).abs().max().item() <= 1e-5
    assert 0 < float(g['sim_err']) < 1e-2
    blk = dec.blocks.group_1.block_1
    assert blk.post_gain == 1 / 64 and blk.res_path.conv_1.kw == 1 and blk.res_path.conv_4.kw == 3
    assert blk.res_path.conv_4.n_out == 2048 and dec.blocks.input.use_float16 is False


def test_unmap_pixels_inverts_map_pixels_and_clamps():
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 3, 5, 7, generator=g)
    assert (dvae.unmap_pixels(dvae.map_pixels(x)) - x).abs().max().item() <= 4 * torch.finfo(torch.float32).eps
    wide = torch.tensor([-3.0, 0.0, 0.1, 0.5, 0.9, 1.0, 7.0]).view(1, 1, 1, 7)
    u = dvae.unmap_pixels(wide)
    assert u.min().item() == 0.0 and u.max().item() == 1.0
    vals = u.flatten().tolist()
    assert vals[:3] == [0.0, 0.0, 0.0] and vals[-2:] == [1.0, 1.0]      # below eps, and above 1 - eps: clamped
    assert abs(vals[3] - 0.5) <= 1e-6 and abs(vals[4] - 1.0) <= 1e-6
    with pytest.raises(ValueError):
        dvae.unmap_pixels(torch.zeros(3, 4, 4))
    with pytest.raises(ValueError):
        dvae.unmap_pixels(torch.zeros(1, 3, 4, 4, dtype=torch.float64))


def test_constructor_validators():
    for bad in (dict(n_init=4), dict(n_hid=32), dict(n_blk_per_group=0), dict(output_channels=0), dict(vocab_size=256)):
        with pytest.raises(ValueError):
            dvae.Decoder(**bad)
    with pytest.raises(ValueError):
        dvae.DecoderBlock(64, 30, 8)
    with pytest.raises(ValueError):
        dvae.DecoderBlock(0, 64, 8)
    with pytest.raises(NotImplementedError):
        dvae.Decoder(group_count=3)


def test_forward_input_checks_come_before_the_device_check():
    """dall_e/decoder.py:127-134: the three ValueErrors are raised for a CPU tensor too."""
    dec = dvae.Decoder(n_hid=64, vocab_size=512)
    with pytest.raises(ValueError, match='4d'):
        dec(torch.zeros(512, 2, 2))
    with pytest.raises(ValueError, match='channels'):
        dec(torch.zeros(1, 100, 2, 2))
    with pytest.raises(ValueError, match='float32'):
        dec(torch.zeros(1, 512, 2, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='cuda'):
        dec(torch.zeros(1, 512, 2, 2))


def _save_under_reference_class_paths(module, path):
    """torch.save of the mirror with the class paths the published pickles carry (dall_e.decoder.Decoder,
    dall_e.decoder.DecoderBlock, dall_e.utils.Conv2d): the mirrors are pickled under temporary stand-in modules."""
    moved = {dvae.Decoder: 'dall_e.decoder', dvae.DecoderBlock: 'dall_e.decoder', dvae.Conv2d: 'dall_e.utils'}
    fake = {n: types.ModuleType(n) for n in ('dall_e', 'dall_e.decoder', 'dall_e.utils')}
    assert not any(n in sys.modules for n in fake)
    old = {c: c.__module__ for c in moved}
    try:
        for c, mod in moved.items():
            c.__module__ = mod
            setattr(fake[mod], c.__name__, c)
        sys.modules.update(fake)
        torch.save(module, path)
    finally:
        for c, mod in old.items():
            c.__module__ = mod
        for n in fake:
            sys.modules.pop(n, None)


def test_dalle_vae_loads_decoder_pkl(tmp_path):
    kw = dict(n_hid=64, vocab_size=512)
    src = dvae.Decoder(**kw)
    sd = synth.synth_dvae_decoder_state_dict(0, **kw)
    src.load_state_dict(sd, strict=True)
    _save_under_reference_class_paths(src, str(tmp_path / 'decoder.pkl'))
    raw = open(tmp_path / 'decoder.pkl', 'rb').read()
    if raw[:2] == b'PK':        # zip container: the pickle stream is the member data.pkl
        import zipfile
        with zipfile.ZipFile(tmp_path / 'decoder.pkl') as zf:
            raw = zf.read([n for n in zf.namelist() if n.endswith('data.pkl')][0])
    assert b'dall_e.decoder' in raw and b'dall_e.utils' in raw and b'exploremultimodal_amd' not in raw
    shutil.copy(ENC_PKL, tmp_path / 'encoder.pkl')
    vae = dvae.create_d_vae(str(tmp_path), 'dall-e', image_size=16, device='cpu')
    assert type(vae.encoder) is dvae.Encoder and type(vae.decoder) is dvae.Decoder
    assert not [n for n in sys.modules if n == 'dall_e' or n.startswith('dall_e.')], 'stand-in modules leaked'
    assert vae.decoder.vocab_size == 512 and vae.decoder.n_init == 128 and vae.decoder.group_count == 4
    got = vae.decoder.state_dict()
    assert list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    assert type(vae.decoder.blocks.group_1.block_1) is dvae.DecoderBlock
    # the engine-side caches work on the unpickled object
    table, bias = vae.decoder.blocks.input.shadow_embed()
    assert table.shape == (512, 128) and torch.equal(table, sd['blocks.input.w'].view(128, 512).t())
    assert torch.equal(bias, sd['blocks.input.b'])
    w4, _ = vae.decoder.blocks.group_4.block_2.res_path.conv_4.shadow()
    assert w4.shape[0] == 64 and w4.dtype == torch.float16


def test_directory_without_decoder_pkl_gives_no_decoder(tmp_path):
    shutil.copy(ENC_PKL, tmp_path / 'encoder.pkl')
    vae = dvae.create_d_vae(str(tmp_path), 'dall-e', image_size=16, device='cpu')
    assert vae.decoder is None
    with pytest.raises(RuntimeError, match='decoder.pkl'):
        vae.decode(torch.zeros(1, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='with_decoder'):
        vae(torch.zeros(1, 4, 512))


def test_create_d_vae_builds_a_decoder_only_on_request():
    vae = dvae.create_d_vae(None, 'dall-e', 112, 'cpu')
    assert vae.decoder is None
    assert not [k for k in vae.state_dict() if k.startswith('decoder.')]
    n_enc = sum(p.numel() for p in vae.parameters())
    vae2 = dvae.create_d_vae(None, 'dall-e', 112, 'cpu', with_decoder=True)
    assert type(vae2.decoder) is dvae.Decoder and vae2.decoder.vocab_size == 8192
    assert sum(p.numel() for p in vae2.parameters()) - n_enc == sum(p.numel() for p in vae2.decoder.parameters()) > 40e6


def test_shadow_embed_follows_the_weight():
    c = dvae.Conv2d(512, 64, 1, use_float16=False)
    t0, _ = c.shadow_embed()
    assert c.shadow_embed()[0] is t0                      # cached
    with torch.no_grad():
        c.w.mul_(2.0)
    t1, _ = c.shadow_embed()
    assert t1 is not t0 and torch.equal(t1, c.w.detach().view(64, 512).t())
    with pytest.raises(ValueError):
        dvae.Conv2d(64, 64, 3).shadow_embed()
