"""Wiring of the attention maps: VLMO.attention_maps, VlmoModule.attention_maps and Block.forward(return_attn=True)
against maps built from the oracle's own functions under oracle.bf16_operands(): per layer attention(...)[1] on
layer_norm of the running activations, then block to advance.

`small` preset (d 256, 4 heads, 3 layers, fusion layer 2, T 24, P 50), synthetic weights with the q and k rows of every
attn.qkv.weight multiplied by 3: as they are, every map is within 0.03 of uniform and a wrong head, layer or transpose
would pass.  The test first asserts that the oracle maps ARE informative (they differ from their head-rolled, transposed,
batch-rolled and neighbouring-layer versions by more than 10x the tolerance).

Tolerance, per layer: twice max |P_oracle(bf16 operands) - P_oracle(fp32)| -- both terms are the oracle, neither is the
code under test.  The engine differs from the bf16-operand oracle by the same kind of event (values that cross a bf16
rounding boundary); the factor 2 covers summation order.  The figures each run finds are printed."""
from functools import partial

import pytest
import torch

from oracle import synth, vlmo_oracle

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GAIN = 3.0
B = 3


def _build(preset, **over):
    from exploremultimodal_amd.vlmo import VLMO, LayerNorm
    mc = synth.make_config(preset, **over).model
    m = VLMO(img_size=mc.img_size, patch_size=mc.patch_size, in_chans=mc.in_chans, num_classes=mc.num_classes,
             embed_dim=mc.embed_dim, depth=mc.depth, num_heads=mc.num_heads, mlp_ratio=mc.mlp_ratio, qkv_bias=mc.qkv_bias,
             norm_layer=partial(LayerNorm, eps=1e-12), init_values=mc.init_values, vocab_size=mc.vocab_size,
             max_text_len=mc.max_text_len, fusion_layer=mc.fusion_layer)
    sd = synth.synth_backbone_state_dict(mc, 0, [('v', 'l', 'vl')] * mc.depth)
    for i in range(mc.depth):
        sd[f'blocks.{i}.attn.qkv.weight'][:2 * mc.embed_dim] *= GAIN
    r = m.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    return m.to(DEV).eval(), mc, sd


def _inputs(mc, batch, mode, dev):
    im = torch.ones(batch['image'].shape[0], synth.num_img_tokens(mc), dtype=torch.int64)
    kw = {}
    if 'img' in mode:
        kw.update(img=batch['image'].to(dev), img_attn_masks=im.to(dev))
    if 'txt' in mode:
        kw.update(txt=batch['text_ids'].to(dev), txt_attn_masks=batch['text_mask'].to(dev))
    return kw


def _oracle_maps(sd, mc, kw, bf16):
    """{layer: map or {'txt', 'img'}} from the oracle's functions, following forward_features (vlmo.py:357-414)."""
    h, maps = mc.num_heads, {}

    def amap(i, x, mask):
        p = f'blocks.{i}.'
        y = vlmo_oracle._ra(vlmo_oracle.layer_norm(x, sd[p + 'norm1.weight'], sd[p + 'norm1.bias']))
        return vlmo_oracle.attention(sd, p + 'attn.', y, mask, h)[1]

    with torch.no_grad(), vlmo_oracle.bf16_operands(bf16):
        img, txt = kw.get('img'), kw.get('txt')
        if txt is None or img is None:
            route, mask = ('v', kw['img_attn_masks']) if txt is None else ('l', kw['txt_attn_masks'])
            x = vlmo_oracle.embed_img(sd, mc, img) if txt is None else vlmo_oracle.embed_txt(sd, mc, txt)
            for i in range(mc.depth):
                maps[i] = amap(i, x, mask)
                x = vlmo_oracle.block(sd, i, x, mask, route, h)
            return maps
        xi, xt = vlmo_oracle.embed_img(sd, mc, img), vlmo_oracle.embed_txt(sd, mc, txt)
        mi, mt = kw['img_attn_masks'], kw['txt_attn_masks']
        for i in range(mc.fusion_layer):
            maps[i] = {'txt': amap(i, xt, mt), 'img': amap(i, xi, mi)}
            xi = vlmo_oracle.block(sd, i, xi, mi, 'v', h)
            xt = vlmo_oracle.block(sd, i, xt, mt, 'l', h)
        x, m = torch.cat([xt, xi], dim=1), torch.cat([mt, mi], dim=1)          # text first: vlmo.py:406
        for i in range(mc.fusion_layer, mc.depth):
            maps[i] = amap(i, x, m)
            x = vlmo_oracle.block(sd, i, x, m, 'vl', h)
    return maps


def _flat(m):
    return m if isinstance(m, dict) else {None: m}


def _layer_tol(bf, fp):
    return 2 * max((a - fp_k).abs().max().item() for a, fp_k in zip(_flat(bf).values(), _flat(fp).values()))


def _assert_informative(maps, tols):
    for i, m in maps.items():
        for kind, P in _flat(m).items():
            others = {'heads rolled': P.roll(1, 1), 'transposed': P.transpose(-1, -2), 'batch rolled': P.roll(1, 0)}
            for j in (i - 1, i + 1):
                Q = _flat(maps[j]).get(kind) if j in maps else None
                if Q is not None and Q.shape == P.shape:
                    others[f'layer {j}'] = Q
            for name, Q in others.items():
                gap = (P - Q).abs().max().item()
                print(f'layer {i} {kind or ""}: {name} differs by {gap:.3f} ({gap / tols[i]:.0f}x the tolerance)')
                assert gap > 10 * tols[i], (i, kind, name, gap, tols[i])


@pytest.fixture(scope='module')
def small():
    model, mc, sd = _build('small')
    batch = synth.synth_batch(mc, B, pad=True)
    return model, mc, sd, batch


@pytest.mark.parametrize('mode', ['img-txt', 'img_only', 'txt_only'])
def test_attention_maps_match_oracle(small, mode):
    model, mc, sd, batch = small
    T, P, H = mc.max_text_len, synth.num_img_tokens(mc), mc.num_heads
    kw_cpu = _inputs(mc, batch, mode, 'cpu')
    bf, fp = _oracle_maps(sd, mc, kw_cpu, True), _oracle_maps(sd, mc, kw_cpu, False)
    tols = {i: _layer_tol(bf[i], fp[i]) for i in bf}
    print(f'{mode}: tolerance per layer (2 x max |P_bf16 - P_fp32| of the oracle): '
          + ', '.join(f'{i}: {t:.2e}' for i, t in tols.items()))
    _assert_informative(bf, tols)
    got = model.attention_maps(**_inputs(mc, batch, mode, DEV))
    assert sorted(got) == list(range(mc.depth))
    for i in range(mc.depth):
        want = _flat(bf[i])
        have = _flat(got[i])
        assert set(have) == set(want), (i, set(have))
        for kind, Pw in want.items():
            Pg = have[kind]
            assert Pg.dtype == torch.float32 and not Pg.requires_grad and Pg.shape == Pw.shape, (i, kind, Pg.shape)
            err = (Pg.cpu() - torch.nan_to_num(Pw)).abs().max().item()
            print(f'{mode} layer {i} {kind or ""}: max |P - P_oracle| {err:.2e} (tolerance {tols[i]:.2e})')
            assert err <= tols[i], (mode, i, kind, err, tols[i])
    if mode == 'img-txt':
        assert got[0]['txt'].shape == (B, H, T, T) and got[0]['img'].shape == (B, H, P, P)
        assert got[mc.fusion_layer].shape == (B, H, T + P, T + P)
        # padded text keys of the odd samples are exactly zero, in the text-first columns of the fused map
        pad = batch['text_mask'] == 0
        assert pad.any()
        assert (got[mc.fusion_layer][:, :, :, :T].cpu()[pad[:, None, None, :].expand(B, H, T + P, T)] == 0).all()
    # a subset of layers gives the same maps; the head mean and a query window are the mean and the slice
    sub = model.attention_maps(layers=[mc.depth - 1], **_inputs(mc, batch, mode, DEV))
    assert list(sub) == [mc.depth - 1] and torch.equal(sub[mc.depth - 1], got[mc.depth - 1])
    win = model.attention_maps(layers=[mc.depth - 1], queries=(1, 5), head_mean=True, **_inputs(mc, batch, mode, DEV))
    ref = got[mc.depth - 1][:, :, 1:6].mean(1, keepdim=True)
    assert win[mc.depth - 1].shape == ref.shape and (win[mc.depth - 1] - ref).abs().max().item() <= 1e-6


def test_block_forward_return_attn(small):
    model, mc, sd, batch = small
    i, N = 1, 37
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, N, mc.embed_dim, generator=g)
    mask = torch.ones(B, N, dtype=torch.int64)
    mask[1, 30:] = 0
    p = f'blocks.{i}.'
    maps = {}
    for bf16 in (True, False):
        with torch.no_grad(), vlmo_oracle.bf16_operands(bf16):
            y = vlmo_oracle._ra(vlmo_oracle.layer_norm(x, sd[p + 'norm1.weight'], sd[p + 'norm1.bias']))
            maps[bf16] = vlmo_oracle.attention(sd, p + 'attn.', y, mask, mc.num_heads)[1]
    tol = 2 * (maps[True] - maps[False]).abs().max().item()
    blk = model.blocks[i]
    out0, none = blk(x.to(DEV), mask.to(DEV), 'vl')
    assert none is None                                         # the default is unchanged
    out1, attn = blk(x.to(DEV), mask.to(DEV), 'vl', return_attn=True)
    assert torch.equal(out0, out1)
    assert attn.shape == (B, mc.num_heads, N, N) and attn.dtype == torch.float32 and not attn.requires_grad
    err = (attn.cpu() - maps[True]).abs().max().item()
    print(f'Block.forward return_attn: max |P - P_oracle| {err:.2e} (tolerance {tol:.2e})')
    assert (maps[True] - maps[True].transpose(-1, -2)).abs().max().item() > 10 * tol
    assert err <= tol
    assert (attn[1, :, :, 30:] == 0).all()


def test_module_attention_maps_equal_the_backbone_call(small):
    from exploremultimodal_amd.build import build_model
    _, mc, sd, batch = small
    cfg = synth.make_config('small')
    module = build_model(cfg)
    keep = {'transformer.' + k: v for k, v in sd.items() if not ('.mlp.vl.' in k and int(k.split('.')[1]) < mc.fusion_layer)}
    r = module.load_state_dict(keep, strict=False)
    assert not r.unexpected_keys and not [k for k in r.missing_keys if k.startswith('transformer.')]
    module = module.to(DEV).eval()
    bd = {k: v.to(DEV) for k, v in batch.items() if torch.is_tensor(v)}
    for mode in ('img-txt', 'img_only', 'txt_only'):
        a = module.attention_maps(bd, infer_mode=mode, layers=[0, 2])
        b = module.transformer.attention_maps(layers=[0, 2], **_inputs(mc, batch, mode, DEV))
        assert sorted(a) == sorted(b) == [0, 2]
        for i in a:
            for kind in _flat(a[i]):
                assert torch.equal(_flat(a[i])[kind], _flat(b[i])[kind]), (mode, i, kind)


def test_training_mode_and_mixed_queries_are_refused(small):
    model, mc, sd, batch = small
    kw = _inputs(mc, batch, 'img-txt', DEV)
    model.train()
    try:
        with pytest.raises(RuntimeError, match='eval'):
            model.attention_maps(**kw)
    finally:
        model.eval()
    with pytest.raises(ValueError, match='queries'):
        model.attention_maps(queries=(0, 1), **kw)              # layers 0 and 1 attend text and image separately
    with pytest.raises(ValueError, match='queries'):
        model.attention_maps(layers=[1, 2], queries=(0, 1), **kw)
    ok = model.attention_maps(layers=[mc.fusion_layer], queries=(0, 1), **kw)
    assert ok[mc.fusion_layer].shape == (B, mc.num_heads, 1, mc.max_text_len + synth.num_img_tokens(mc))
    with pytest.raises(ValueError):
        model.attention_maps(layers=[mc.depth], **kw)


def test_long_path_480px_cls_row_head_mean():
    """mini at 480 px: 917 fused tokens (the kernel's long path), CLS-text query row, mean over heads."""
    model, mc, sd = _build('mini', img_size=480)
    batch = synth.synth_batch(mc, 2, pad=True)
    T, P = mc.max_text_len, synth.num_img_tokens(mc)
    assert T + P == 917
    kw_cpu = _inputs(mc, batch, 'img-txt', 'cpu')
    L = mc.fusion_layer
    bf, fp = (_oracle_maps(sd, mc, kw_cpu, m)[L][:, :, 0:1].mean(1, keepdim=True) for m in (True, False))
    tol = 2 * (bf - fp).abs().max().item()
    got = model.attention_maps(layers=[L], queries=(0, 1), head_mean=True, **_inputs(mc, batch, 'img-txt', DEV))[L]
    assert got.shape == (2, 1, 1, 917)
    err = (got.cpu() - bf).abs().max().item()
    print(f'480 px fused layer, row 0, head mean: max |P - P_oracle| {err:.2e} (tolerance {tol:.2e}); '
          f'row maximum {bf.max().item():.3f} against uniform {1 / 917:.4f}')
    assert (bf - bf.roll(1, 0)).abs().max().item() > 10 * tol
    assert err <= tol
    pad = batch['text_mask'] == 0
    assert (got[:, 0, 0, :T].cpu()[pad] == 0).all()
