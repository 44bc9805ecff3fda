"""Wiring of the gradient-weighted attention maps: VLMO.attention_gradcam and VlmoModule.attention_gradcam against maps
built on the CPU from the oracle's own functions layer_norm, attention and mlp, composed into blocks by hand so that
``attention(...)[1]`` stays in the graph with ``retain_grad()`` -- the hook-and-retain_grad form of the reference -- and
torch autograd of the same score.  The composition follows forward_features (vlmo.py:357-414).

`small` preset (d 256, 4 heads, 3 layers, fusion layer 2, T 24, P 50) with the q and k rows of every attn.qkv.weight
multiplied by 3, as in tests/test_attnmap_module_gpu.py.  The oracle's ``attn.grad`` has dctx . v on masked keys too; the
definition of the maps puts exact zeros there for every kind, so the oracle maps are masked the same way.

Tolerance, per layer, kind and (below the fusion layer) modality: twice max |X_oracle(bf16 operands) - X_oracle(fp32)| of
that very map -- both terms are the oracle, neither is the code under test; the factor 2 is the one that file uses for
summation order.  The score reads the first and the last token, so that both modalities carry gradient below the fusion
layer (with the text CLS alone the image maps of layer 1 are too small to tell from their head-rolled version).  The test first asserts that the
oracle maps ARE informative: they differ from their head-rolled, batch-rolled and transposed versions, and from the plain
attention map scaled to the same norm, by more than 10x the tolerance.  The figures each run finds are printed."""
from functools import partial

import pytest
import torch
import torch.nn.functional as F

from oracle import synth, vlmo_oracle

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GAIN = 3.0
B = 3


def _state(preset, **over):
    mc = synth.make_config(preset, **over).model
    sd = synth.synth_backbone_state_dict(mc, 0, [('v', 'l', 'vl')] * mc.depth)
    for i in range(mc.depth):
        sd[f'blocks.{i}.attn.qkv.weight'][:2 * mc.embed_dim] *= GAIN
    return mc, sd


def _build(preset, **over):
    from exploremultimodal_amd.vlmo import VLMO, LayerNorm
    mc, sd = _state(preset, **over)
    m = VLMO(img_size=mc.img_size, patch_size=mc.patch_size, in_chans=mc.in_chans, num_classes=mc.num_classes,
             embed_dim=mc.embed_dim, depth=mc.depth, num_heads=mc.num_heads, mlp_ratio=mc.mlp_ratio, qkv_bias=mc.qkv_bias,
             norm_layer=partial(LayerNorm, eps=1e-12), init_values=mc.init_values, vocab_size=mc.vocab_size,
             max_text_len=mc.max_text_len, fusion_layer=mc.fusion_layer)
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


def _oracle(sd, mc, kw, score_fn, bf16, layers):
    """{layer: (P, G) or {'txt': (P, G), 'img': (P, G)}} of the requested layers: the oracle's attention maps and the
    gradient torch autograd leaves in them for score_fn(final features), masked keys zeroed."""
    h, kept = mc.num_heads, {}

    def block(i, x, mask, route, name):
        p = f'blocks.{i}.'
        y = vlmo_oracle._ra(vlmo_oracle.layer_norm(x, sd[p + 'norm1.weight'], sd[p + 'norm1.bias']))
        a, attn = vlmo_oracle.attention(sd, p + 'attn.', y, mask, h)
        if i in layers:
            attn.retain_grad()
            kept.setdefault(i, {})[name] = (attn, mask)
        x = x + sd[p + 'gamma_1'] * a if p + 'gamma_1' in sd else x + a
        y = vlmo_oracle._ra(vlmo_oracle.layer_norm(x, sd[p + 'norm2.weight'], sd[p + 'norm2.bias']))
        m = vlmo_oracle.mlp(sd, p + f'mlp.{route}.', y)
        return x + sd[p + 'gamma_2'] * m if p + 'gamma_2' in sd else x + m

    with vlmo_oracle.bf16_operands(bf16):
        img, txt = kw.get('img'), kw.get('txt')
        with torch.no_grad():
            xi = vlmo_oracle.embed_img(sd, mc, img) if img is not None else None
            xt = vlmo_oracle.embed_txt(sd, mc, txt) if txt is not None else None
        if txt is None or img is None:
            route, mask = ('v', kw['img_attn_masks']) if txt is None else ('l', kw['txt_attn_masks'])
            x = (xi if txt is None else xt).requires_grad_(True)
            for i in range(mc.depth):
                x = block(i, x, mask, route, None)
        else:
            xi, xt = xi.requires_grad_(True), xt.requires_grad_(True)
            mi, mt = kw['img_attn_masks'], kw['txt_attn_masks']
            for i in range(mc.fusion_layer):
                xi = block(i, xi, mi, 'v', 'img')
                xt = block(i, xt, mt, 'l', 'txt')
            x, mask = torch.cat([xt, xi], dim=1), torch.cat([mt, mi], dim=1)      # text first: vlmo.py:406
            for i in range(mc.fusion_layer, mc.depth):
                x = block(i, x, mask, 'vl', None)
        out = vlmo_oracle.layer_norm(x, sd['norm.weight'], sd['norm.bias'])
        score_fn(out).backward()
    res = {}
    for i, d in kept.items():
        pg = {name: (a.detach(), a.grad * (m != 0)[:, None, None, :]) for name, (a, m) in d.items()}
        res[i] = pg[None] if None in pg else pg
    return res


def _kind(P, G, kind):
    return {'grad': G, 'attn_grad': P * G, 'cam': P * G.clamp_min(0)}[kind]


def _flat(m):
    return m if isinstance(m, dict) else {None: m}


def _maps(pg, kind):
    return {i: ({n: _kind(*v, kind) for n, v in m.items()} if isinstance(m, dict) else _kind(*m, kind))
            for i, m in pg.items()}


def _tolerances(bf, fp):
    """{(layer, 'txt' | 'img' | None): 2 max |X_bf16 - X_fp32|}: every map is held to its own oracle error."""
    return {(i, n): 2 * (a - _flat(fp[i])[n]).abs().max().item() for i in bf for n, a in _flat(bf[i]).items()}


def _assert_informative(maps, pg, tols, what):
    for i, m in maps.items():
        for name, X in _flat(m).items():
            P = _flat(pg[i])[name][0]
            others = {'heads rolled': X.roll(1, 1), 'transposed': X.transpose(-1, -2), 'batch rolled': X.roll(1, 0),
                      'the plain map at the same norm': P * (X.norm() / P.norm())}
            for oname, Q in others.items():
                gap = (X - Q).abs().max().item()
                print(f'{what} layer {i} {name or ""}: {oname} differs by {gap:.3e} ({gap / tols[i, name]:.0f}x the tolerance)')
                assert gap > 10 * tols[i, name], (what, i, name, oname, gap, tols[i, name])


def _compare(got, want, tols, what):
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for i in want:
        have, ref = _flat(got[i]), _flat(want[i])
        assert set(have) == set(ref), (i, set(have))
        for name, X in ref.items():
            Y = have[name]
            assert Y.dtype == torch.float32 and not Y.requires_grad and Y.grad_fn is None and Y.shape == X.shape, (i, Y.shape)
            err = (Y.cpu() - X).abs().max().item()
            print(f'{what} layer {i} {name or ""}: max |X - X_oracle| {err:.3e} (tolerance {tols[i, name]:.3e}, '
                  f'max |X_oracle| {X.abs().max().item():.3e})')
            assert err <= tols[i, name], (what, i, name, err, tols[i, name])


def _weights(mc):
    return torch.randn(2, mc.embed_dim, generator=torch.Generator().manual_seed(11))


def _score(w):
    """A callable score with fixed weights: the first token (the text CLS, or the image CLS of an image-only pass) and the
    last one (an image patch), so that below the fusion layer both modalities carry gradient."""
    return lambda x, mask=None: (x[:, 0] @ w[0] + x[:, -1] @ w[1]).sum()


@pytest.fixture(scope='module')
def small():
    model, mc, sd = _build('small')
    batch = synth.synth_batch(mc, B, pad=True)
    return model, mc, sd, batch


@pytest.fixture(scope='module')
def oracle_cases(small):
    """The oracle's (P, G) per mode, computed once: {mode: (bf16-operand, fp32)} for the callable score
    _score(w) with fixed weights."""
    _, mc, sd, batch = small
    w = _weights(mc)
    out = {}
    for mode, layers in (('img-txt', [1, 2]), ('img_only', [0, 2])):
        kw = _inputs(mc, batch, mode, 'cpu')
        out[mode] = tuple(_oracle(sd, mc, kw, _score(w), bf, layers) for bf in (True, False))
    return out


@pytest.mark.parametrize('kind', ['cam', 'grad'])
@pytest.mark.parametrize('mode', ['img-txt', 'img_only'])
def test_gradcam_matches_oracle_autograd(small, oracle_cases, mode, kind):
    model, mc, sd, batch = small
    T, P, H = mc.max_text_len, synth.num_img_tokens(mc), mc.num_heads
    bf, fp = oracle_cases[mode]
    want, tols = _maps(bf, kind), _tolerances(_maps(bf, kind), _maps(fp, kind))
    _assert_informative(want, bf, tols, f'{mode} {kind}')
    w = _weights(mc).to(DEV)
    got = model.attention_gradcam(_score(w), layers=sorted(want), kind=kind,
                                  **_inputs(mc, batch, mode, DEV))
    _compare(got, want, tols, f'{mode} {kind}')
    if mode == 'img-txt':
        L = mc.fusion_layer
        assert got[1]['txt'].shape == (B, H, T, T) and got[1]['img'].shape == (B, H, P, P)
        assert got[L].shape == (B, H, T + P, T + P)
        pad = batch['text_mask'] == 0
        assert pad.any()                 # padded text keys are exactly zero in the text-first columns, for every kind
        assert (got[L][:, :, :, :T].cpu()[pad[:, None, None, :].expand(B, H, T + P, T)] == 0).all()
        # the head mean and a query window are the mean and the slice
        win = model.attention_gradcam(_score(w), layers=[L], kind=kind, queries=(1, 5),
                                      head_mean=True, **_inputs(mc, batch, mode, DEV))[L]
        ref = got[L][:, :, 1:6].mean(1, keepdim=True)
        assert win.shape == ref.shape and (win - ref).abs().max().item() <= 1e-6 * max(1.0, ref.abs().max().item())


def _build_module(mc, sd, losses):
    from exploremultimodal_amd.build import build_model
    module = build_model(synth.make_config('small', loss_names=losses))
    keep = {'transformer.' + k: v for k, v in sd.items() if not ('.mlp.vl.' in k and int(k.split('.')[1]) < mc.fusion_layer)}
    heads = synth.synth_head_state_dict(mc, 0, losses)
    keep.update(heads)
    r = module.load_state_dict(keep, strict=False)
    assert not r.unexpected_keys and not [k for k in r.missing_keys if k.startswith(('transformer.', 'itm_head.'))]
    return module.to(DEV).eval(), heads


def test_module_itm_target_matches_oracle(small):
    """target='itm': the match logit itm_head(pooler(x))[:, 1] summed over the batch, against the same composition with
    the ITM head on the pooled CLS."""
    _, mc, sd, batch = small
    module, heads = _build_module(mc, sd, ['itm'])
    L = mc.fusion_layer
    kw = _inputs(mc, batch, 'img-txt', 'cpu')

    def score(x):
        return F.linear(vlmo_oracle.pooler(sd, x), heads['itm_head.fc.weight'], heads['itm_head.fc.bias'])[:, 1].sum()

    bf, fp = (_oracle(sd, mc, kw, score, m, [L]) for m in (True, False))
    bd = {k: v.to(DEV) for k, v in batch.items() if torch.is_tensor(v)}
    for kind in ('cam', 'grad'):
        want, tols = _maps(bf, kind), _tolerances(_maps(bf, kind), _maps(fp, kind))
        _assert_informative(want, bf, tols, f'itm {kind}')
        got = module.attention_gradcam(bd, layers=[L], kind=kind)
        _compare(got, want, tols, f'itm {kind}')
    # a callable target gets the dict infer returns
    a = module.attention_gradcam(bd, layers=[L], target=lambda out: module.itm_head(out['cls_feats'])[:, 1].sum())
    assert torch.equal(a[L], module.attention_gradcam(bd, layers=[L])[L])
    # a model without the ITM head refuses the target
    plain, _ = _build_module(mc, sd, [])
    with pytest.raises(ValueError, match='itm'):
        plain.attention_gradcam(bd, layers=[L])
    module.train()
    try:
        with pytest.raises(RuntimeError, match='eval'):
            module.attention_gradcam(bd, layers=[L])
    finally:
        module.eval()


def test_long_path_480px_text_rows_head_mean():
    """mini at 480 px: 917 fused tokens (the kernel's 513 - 1024 arrangement and the streaming attention backward), the
    text rows against every key, mean over heads."""
    from exploremultimodal_amd import attnmap
    model, mc, sd = _build('mini', img_size=480)
    batch = synth.synth_batch(mc, 2, pad=True)
    T, P = mc.max_text_len, synth.num_img_tokens(mc)
    assert T + P == 917
    L = mc.fusion_layer
    w = _weights(mc)
    kw_cpu = _inputs(mc, batch, 'img-txt', 'cpu')
    bf, fp = ({L: _kind(*_oracle(sd, mc, kw_cpu, _score(w), m, [L])[L], 'cam')[:, :, :T]
               .mean(1, keepdim=True)} for m in (True, False))
    tols = _tolerances(bf, fp)
    wd = w.to(DEV)
    got = model.attention_gradcam(_score(wd), layers=[L], queries=(0, T), head_mean=True,
                                  **_inputs(mc, batch, 'img-txt', DEV))
    assert got[L].shape == (2, 1, T, 917)
    assert (bf[L] - bf[L].roll(1, 0)).abs().max().item() > 10 * tols[L, None]
    _compare(got, bf, tols, '480 px cam head mean')
    pad = batch['text_mask'] == 0
    assert (got[L][:, 0, :, :T].cpu()[pad[:, None, :].expand(2, T, T)] == 0).all()
    grid = mc.img_size // mc.patch_size
    hm = attnmap.text_to_image_heatmaps(got[L], T, grid)
    assert hm.shape == (2, 1, T, grid, grid) and torch.equal(hm.reshape(2, 1, T, -1), got[L][:, :, :, T + 1:])


def test_no_side_effects(small):
    """A call leaves every p.grad (the very tensor), every requires_grad flag and model.training as they were, and the
    gradients of a plain eval-mode backward taken before and after it are bitwise equal.

    Bitwise holds for the gradients the engine sums in a fixed order: the weight matrices of the blocks (stored by the
    weight-gradient GEMMs).  The vector gradients of the blocks (column folds) and the embedding tables are summed with
    fp32 atomics: two plain passes differ there with no call in between (measured on an MI355X, `small`, 3 pairs: 6 - 7 of
    65 parameters, by 1.5 - 4.3 u of the parameter's largest element, e.g. 6.1e-5 at 622.8 for
    txt_embeddings.token_type_embeddings.weight), so bitwise equality cannot be asked of them.  They are held to 1e-5 of
    the parameter's largest gradient element: a reordered fp32 sum of n terms moves by at most 2 n u sum |t|, and sum |t|
    is not observable from outside, so this stands in for it (40x the spread measured between plain passes; any state the
    call left behind would also move the matrices, which are compared bitwise)."""
    model, mc, sd, batch = small
    kw = _inputs(mc, batch, 'img-txt', DEV)
    w = _weights(mc).to(DEV)

    def plain_grads():
        model.zero_grad(set_to_none=True)
        model.forward_features(**kw)[0].sum().backward()
        return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    before = plain_grads()
    fixed_order = [n for n, g in before.items() if n.startswith('blocks.') and g.dim() == 2]
    assert len(fixed_order) >= 4 * mc.depth
    flags = {n: p.requires_grad for n, p in model.named_parameters()}
    held = {n: p.grad for n, p in model.named_parameters()}
    model.attention_gradcam(_score(w), layers=[0, mc.fusion_layer], **kw)
    assert not model.training
    for n, p in model.named_parameters():
        assert p.requires_grad == flags[n], n
        assert p.grad is held[n], n                             # the very tensor (or None) it held before the call
        if p.grad is not None:
            assert torch.equal(p.grad, before[n]), n
    after = plain_grads()
    assert set(after) == set(before)
    for n in fixed_order:
        assert torch.equal(after[n], before[n]), n
    moved = {n: (after[n] - before[n]).abs().max().item() for n in before if not torch.equal(after[n], before[n])}
    print(f'{len(before) - len(moved)} of {len(before)} gradients bitwise equal; atomically summed ones moved by', moved)
    for n, dlt in moved.items():
        assert dlt <= 1e-5 * before[n].abs().max().item(), (n, dlt)
    # every parameter frozen: the embedded input is the leaf
    try:
        for p in model.parameters():
            p.requires_grad_(False)
        frozen = model.attention_gradcam(_score(w), layers=[mc.fusion_layer], **kw)
    finally:
        for n, p in model.named_parameters():
            p.requires_grad_(flags[n])
    live = model.attention_gradcam(_score(w), layers=[mc.fusion_layer], **kw)
    assert torch.equal(frozen[mc.fusion_layer], live[mc.fusion_layer])


def test_refusals(small):
    from exploremultimodal_amd import engine
    model, mc, sd, batch = small
    kw = _inputs(mc, batch, 'img-txt', DEV)
    w = _weights(mc).to(DEV)
    score = _score(w)
    model.train()
    try:
        with pytest.raises(RuntimeError, match='eval'):
            model.attention_gradcam(score, **kw)
    finally:
        model.eval()
    with pytest.raises(ValueError, match='queries'):
        model.attention_gradcam(score, queries=(0, 1), **kw)    # layers 0 and 1 attend text and image separately
    with pytest.raises(ValueError, match='queries'):
        model.attention_gradcam(score, layers=[1, 2], queries=(0, 1), **kw)
    with pytest.raises(ValueError):
        model.attention_gradcam(score, layers=[mc.depth], **kw)
    with pytest.raises(ValueError, match='kind'):
        model.attention_gradcam(score, kind='gradcam', **kw)
    for bad in (lambda x, mask: x[:, 0] @ w[0], lambda x, mask: x.sum().detach(), lambda x, mask: 1.0):
        with pytest.raises(ValueError, match='scalar'):
            model.attention_gradcam(bad, layers=[mc.fusion_layer], **kw)

    class Sink:                                                 # any attached reducer: the call must not reach it
        def __getattr__(self, name):
            raise AssertionError(f'the gradient reducer was handed {name}')

    engine.GRAD_SINK = Sink()
    try:
        with pytest.raises(RuntimeError, match='reducer'):
            model.attention_gradcam(score, layers=[mc.fusion_layer], **kw)
    finally:
        engine.GRAD_SINK = None
