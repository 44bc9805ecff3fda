"""dVAE decoder on the HIP engine: the four decoder kernels one by one (token embedding, nearest 2x upsampling, the 3x3
block tail with the residual epilogue, the six-channel output head), the reordering of upsampling and 1x1 convolutions,
and the whole decoder against the reference's fp32 output (tests/golden/dvae_dec_*.npz).

End-to-end bound: max |y_hip - y| <= 4 * sim_err, sim_err from the fixture = the reference's own error when its
convolution operands are rounded to fp16 (tools/gen_decoder_golden.py).  The factor 4 covers the fused tails (one
rounding where the emulation has two) and the MFMA summation order.  Each end-to-end test prints the observed ratio;
on an MI355X: 1.42 (small, decode_ids), 1.21 (small, forward on the one-hot map), 1.52 (full)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from exploremultimodal_amd import dvae, hip, synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F16 = torch.float16


def _nhwc(x):      # [B,C,H,W] -> [B*H*W, C]
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


def _nchw(m, B, H, W):      # [B*H*W, C] -> [B,C,H,W]
    return m.view(B, H, W, -1).permute(0, 3, 1, 2)


def _w3(w):        # [Cout, Cin, 3, 3] -> the engine's [Cout, 9*Cin], tap-major
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


_DECODERS = {}


def _decoder(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _DECODERS:
        dec = dvae.Decoder(**kw)
        dec.load_state_dict(synth.synth_dvae_decoder_state_dict(0, **kw), strict=True)
        _DECODERS[key] = dec.to(DEV)
    return _DECODERS[key]


# ---------------------------------------------------------------- embed
def test_embed_is_the_rounded_table_row_plus_bias():
    M, vocab, n_init = 37, 512, 128
    g = torch.Generator().manual_seed(11)
    table = torch.randn(vocab, n_init, generator=g).to(DEV)
    bias = torch.randn(n_init, generator=g).to(DEV)
    ids = torch.randint(0, vocab, (M,), generator=g)
    ids[0], ids[1], ids[-1] = 0, 511, 511
    ids = ids.to(DEV)
    out = torch.full((M, n_init), float('nan'), dtype=F16, device=DEV)
    hip.dvae_embed(ids, table, bias, out)
    assert torch.equal(out, (table[ids] + bias).half())


def test_decode_ids_rejects_bad_ids():
    dec = _decoder(n_hid=256, vocab_size=1024)
    ok = torch.zeros(1, 2, 2, dtype=torch.int64, device=DEV)
    for bad in (1024, -1):
        ids = ok.clone()
        ids[0, 1, 1] = bad
        with pytest.raises(ValueError, match='ids must lie'):
            dec.decode_ids(ids)
    with pytest.raises(ValueError):
        dec.decode_ids(ok.int())
    with pytest.raises(ValueError):
        dec.decode_ids(ok[0])


# ---------------------------------------------------------------- upsample
@pytest.mark.parametrize('B,H,W,C', [(2, 3, 5, 64), (1, 1, 1, 8), (2, 4, 4, 1280)])
def test_upsample2_equals_interpolate_nearest(B, H, W, C):
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, C, H, W, generator=g).half().to(DEV)
    out = torch.full((B * 4 * H * W, C), float('nan'), dtype=F16, device=DEV)
    hip.upsample2_nhwc(_nhwc(x), out, B, H, W, C)
    ref = F.interpolate(x.float(), scale_factor=2, mode='nearest').half()
    assert torch.equal(_nchw(out, B, 2 * H, 2 * W), ref)
    with pytest.raises(RuntimeError, match='multiple of 8'):
        hip.upsample2_nhwc(out, out, 1, 1, 1, 12)


# ---------------------------------------------------------------- tail
@pytest.mark.parametrize('with_out2', [True, False])
def test_tail_exact_integers_borders(with_out2):
    """3x3 convolution with the residual epilogue on integer data (exact sums, beta a power of two): 60 rows = one ragged
    row tile, every image border, two 128-channel column tiles."""
    B, H, W, Cin, Cout = 2, 5, 6, 64, 256
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-2, 3, (B, Cin, H, W), generator=g).float()
    w = torch.randint(-1, 2, (Cout, Cin, 3, 3), generator=g).float()
    bias = torch.randint(-4, 5, (Cout,), generator=g).float()
    resid = torch.randint(-8, 9, (B, Cout, H, W), generator=g).float()
    ref = (resid + (F.conv2d(x, w, bias, padding=1)) / 64).half()
    out = torch.full((B * H * W, Cout), float('nan'), dtype=F16, device=DEV)
    out2 = torch.full_like(out, float('nan')) if with_out2 else None
    hip.conv2d_nhwc(hip.EPI_DUAL, _nhwc(x.half().to(DEV)), B, H, W, Cin, 3, _w3(w).half().to(DEV), Cout, out, out2=out2,
                    bias=bias.to(DEV), resid=_nhwc(resid.half().to(DEV)), beta=1 / 64)
    assert torch.equal(_nchw(out, B, H, W).cpu(), ref)
    if with_out2:
        assert torch.equal(_nchw(out2, B, H, W).cpu(), ref.relu())


@pytest.mark.parametrize('B,H,W,Cin,Cout', [(1, 4, 4, 512, 2048),      # group 1 of the decoder
                                            (2, 9, 11, 64, 32)])       # ragged channel tile of the 256 x 64 kernel
def test_tail_random_vs_torch(B, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(Cin + Cout)
    x = torch.randn(B, Cin, H, W, generator=g).half().to(DEV)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).half().to(DEV)
    b = torch.randn(Cout, generator=g).to(DEV)
    resid = torch.randn(B, Cout, H, W, generator=g).half().to(DEV)
    beta = 1 / 64
    ref = resid.float() + beta * F.conv2d(x.float(), w.float(), b, padding=1)
    out, out2 = (torch.full((B * H * W, Cout), float('nan'), dtype=F16, device=DEV) for _ in range(2))
    hip.conv2d_nhwc(hip.EPI_DUAL, _nhwc(x), B, H, W, Cin, 3, _w3(w), Cout, out, out2=out2, bias=b, resid=_nhwc(resid),
                    beta=beta)
    tol = 4e-3 + 2e-3 * ref.abs().max().item()
    err = (_nchw(out, B, H, W).float() - ref).abs().max().item()
    err2 = (_nchw(out2, B, H, W).float() - ref.relu()).abs().max().item()
    print(f'tail {B}x{H}x{W} {Cin}->{Cout}: err {err:.3g} relu err {err2:.3g} tol {tol:.3g}')
    assert err <= tol and err2 <= tol
    # relu on the input fragments and no residual (resid = NULL reads as 0)
    ref3 = beta * F.conv2d(x.float().relu(), w.float(), b, padding=1)
    hip.conv2d_nhwc(hip.EPI_DUAL, _nhwc(x), B, H, W, Cin, 3, _w3(w), Cout, out, bias=b, beta=beta, relu_in=True)
    assert (_nchw(out, B, H, W).float() - ref3).abs().max().item() <= 4e-3 + 2e-3 * ref3.abs().max().item()


# ---------------------------------------------------------------- output head
@pytest.mark.parametrize('B,H,W,C,Cout', [(2, 7, 9, 256, 6), (1, 1, 3, 64, 2)])
def test_out_head_exact_integers_nchw(B, H, W, C, Cout):
    g = torch.Generator().manual_seed(C + Cout)
    x = torch.randint(-3, 4, (B, C, H, W), generator=g).float()
    w = torch.randint(-2, 3, (Cout, C, 1, 1), generator=g).float()
    b = torch.randint(-5, 6, (Cout,), generator=g).float()
    ref = F.conv2d(x.relu(), w, b)
    out = torch.full((B, Cout, H, W), float('nan'), device=DEV)
    hip.dvae_out_head(_nhwc(x.half().to(DEV)), w.view(Cout, C).half().to(DEV), b.to(DEV), out, B, H, W)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (B, Cout, H, W)
    assert torch.equal(out.cpu(), ref)
    assert (ref != F.conv2d(x, w, b)).any(), 'the case must tell relu(x) from x'
    with pytest.raises(RuntimeError, match='Cout'):
        hip.dvae_out_head(_nhwc(x.half().to(DEV)), torch.zeros(9, C, dtype=F16, device=DEV), torch.zeros(9, device=DEV),
                          torch.zeros(B, 9, H, W, device=DEV), B, H, W)


# ---------------------------------------------------------------- reordering
def test_upsampling_commutes_with_the_blocks_1x1_convolutions():
    """block_1 of group 2 (n_hid=256: 2048 -> 1024, bottleneck 256) on a [2, 4, 4, 2048] map: upsample-then-1x1 (the
    reference's order, decoder.py:85 then 30-37) and 1x1-then-upsample (Decoder._body) give the same bits: per pixel
    the same products in the same order."""
    dec = _decoder(n_hid=256, vocab_size=1024)
    blk = dec.blocks.group_2.block_1
    B, H, W, C = 2, 4, 4, 2048
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B * H * W, C, generator=g).half().to(DEV)
    em = lambda m, c: torch.full((m, c), float('nan'), dtype=F16, device=DEV)
    M = B * H * W

    def convs(src, h, w):
        m = B * h * w
        w1, b1 = blk.res_path.conv_1.shadow()
        wi, bi = blk.id_path.shadow()
        t, idp = em(m, blk.n_hid), em(m, blk.n_out)
        hip.conv2d_nhwc(hip.EPI_BIAS, src, B, h, w, C, 1, w1, blk.n_hid, t, bias=b1, relu=True, relu_in=True)
        hip.conv2d_nhwc(hip.EPI_BIAS, src, B, h, w, C, 1, wi, blk.n_out, idp, bias=bi)
        return t, idp

    xu = em(4 * M, C)
    hip.upsample2_nhwc(x, xu, B, H, W, C)
    t_a, id_a = convs(xu, 2 * H, 2 * W)
    t_lo, id_lo = convs(x, H, W)
    t_b, id_b = em(4 * M, blk.n_hid), em(4 * M, blk.n_out)
    hip.upsample2_nhwc(t_lo, t_b, B, H, W, blk.n_hid)
    hip.upsample2_nhwc(id_lo, id_b, B, H, W, blk.n_out)
    assert torch.equal(t_a, t_b) and torch.equal(id_a, id_b)
    assert t_a.float().abs().max().item() > 0.1 and (t_a >= 0).all()


# ---------------------------------------------------------------- end to end
def _ratio(name, y, g):
    ref = torch.from_numpy(g['y'])
    sim = float(g['sim_err'])
    err = (y.cpu() - ref).abs().max().item()
    print(f'{name}: max|y_hip - y| = {err:.4g}, sim_err = {sim:.4g}, ratio = {err / sim:.3f} (bound 4), '
          f'max|y| = {ref.abs().max().item():.4g}')
    return err, sim


def test_decoder_small_matches_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, 'dvae_dec_small.npz'))
    dec = _decoder(n_hid=256, vocab_size=1024)
    ids = torch.from_numpy(g['ids']).to(DEV)
    y = dec.decode_ids(ids)
    assert y.shape == (2, 6, 32, 32) and y.dtype == torch.float32 and y.is_contiguous()
    err, sim = _ratio('dvae_dec_small decode_ids', y, g)
    # Decoder.forward on the explicit one-hot map: the dense input convolution
    z = F.one_hot(ids, num_classes=1024).permute(0, 3, 1, 2).float()
    yz = dec(z)
    errz, _ = _ratio('dvae_dec_small forward(one-hot)', yz, g)
    assert err <= 4 * sim
    assert errz <= 4 * sim
    with pytest.raises(ValueError, match='4d'):
        dec(z[0])
    with pytest.raises(ValueError, match='channels'):
        dec(z[:, :512])
    with pytest.raises(ValueError, match='float32'):
        dec(z.double())
    # the wrapper: flat token sequences, as the MIM head predicts them
    vae = dvae.Dalle_VAE(32)
    vae.decoder = dec
    yv = vae.decode(ids.view(2, 16))
    assert torch.equal(yv, y)
    probs = F.one_hot(ids.view(2, 16), num_classes=1024).float()
    assert torch.equal(vae(probs), yz) and torch.equal(vae(z, no_process=True), yz)
    img = dvae.unmap_pixels(torch.sigmoid(yv[:, :3]))
    assert img.shape == (2, 3, 32, 32) and 0 <= img.min().item() and img.max().item() <= 1


def test_decoder_full_matches_reference(golden_dir):
    """Default model, ids [2, 14, 14] -> [2, 6, 112, 112]."""
    g = np.load(os.path.join(golden_dir, 'dvae_dec_full_b2.npz'))
    dec = _decoder()
    y = dec.decode_ids(torch.from_numpy(g['ids']).to(DEV))
    assert y.shape == (2, 6, 112, 112)
    err, sim = _ratio('dvae_dec_full_b2 decode_ids', y, g)
    assert err <= 4 * sim
