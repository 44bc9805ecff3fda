"""Wiring of VLMO.attention_relevance and VlmoModule.attention_relevance: every result against
attnmap.relevance_reference(..., dtype=float64) over the head-mean maps that attention_gradcam(kind='cam', head_mean=True) /
attention_maps(head_mean=True) return for the same model, inputs and layers -- those calls run the very launches the
relevance pass runs and are bitwise reproducible, so the only difference is the propagation (vlmo_relevance_step in fp32,
rows from the top layer down, against the fp64 matrix recursion from the bottom layer up).

`small` preset as in tests/test_gradcam_module_gpu.py (d 256, 4 heads, 3 layers, fusion layer 2 -- strictly inside the
depth --, T 24, P 50, padded text) with the q and k rows of every attn.qkv.weight multiplied by 3.

Bound, as for the kernel (tests/test_relevance_gpu.py): every term is >= 0, a step is at most N + 2 roundings of 2^-24,
doubled for the MFMA's inner accumulation: per element a RELATIVE error of at most L (N + 3) 2^-23 with N the token count
of the pass, and exactly 0 wherever fp64 is exactly 0 (the columns of padded text keys off the diagonal).

queries: None, (0, 1) and (T - 1, 3) -- the last text token, the image CLS and the first patch of an image-text pass.  In an
image-only pass (N = P = 50 > T + 2) the same window is valid; in a text-only pass N = T, the window leaves [0, N] and is one
of the refusals, so the window there is the last three tokens (T - 3, 3) and (T - 1, 3) is asserted to raise."""

import pytest
import torch

from exploremultimodal_amd import attnmap
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GAIN = 3.0
B = 3
MODES = {'img-txt': ('img', 'txt'), 'img_only': ('img',), 'txt_only': ('txt',)}


@pytest.fixture(scope='module')
def small():
    """(VlmoModule with the ITM head in eval mode on the GPU, model config, batch on the GPU)."""
    from exploremultimodal_amd.build import build_model
    mc = synth.make_config('small').model
    sd = synth.synth_backbone_state_dict(mc, 0, [('v', 'l', 'vl')] * mc.depth)
    for i in range(mc.depth):
        sd[f'blocks.{i}.attn.qkv.weight'][:2 * mc.embed_dim] *= GAIN
    module = build_model(synth.make_config('small', loss_names=['itm']))
    keep = {'transformer.' + k: v for k, v in sd.items() if not ('.mlp.vl.' in k and int(k.split('.')[1]) < mc.fusion_layer)}
    keep.update(synth.synth_head_state_dict(mc, 0, ['itm']))
    r = module.load_state_dict(keep, strict=False)
    assert not r.unexpected_keys and not [k for k in r.missing_keys if k.startswith(('transformer.', 'itm_head.'))]
    assert 0 < mc.fusion_layer < mc.depth
    batch = synth.synth_batch(mc, B, pad=True)
    assert (batch['text_mask'] == 0).any()
    bd = {k: v.to(DEV) for k, v in batch.items() if torch.is_tensor(v)}
    return module.to(DEV).eval(), mc, bd


def _kw(mc, bd, mode):
    kw = {}
    if 'img' in MODES[mode]:
        kw.update(img=bd['image'], img_attn_masks=torch.ones(B, synth.num_img_tokens(mc), dtype=torch.int64, device=DEV))
    if 'txt' in MODES[mode]:
        kw.update(txt=bd['text_ids'], txt_attn_masks=bd['text_mask'])
    return kw


def _score(mc):
    w = torch.randn(2, mc.embed_dim, generator=torch.Generator().manual_seed(11)).to(DEV)
    return lambda x, mask=None: (x[:, 0] @ w[0] + x[:, -1] @ w[1]).sum()


def _sizes(mc, mode):
    T = mc.max_text_len if 'txt' in MODES[mode] else 0
    P = synth.num_img_tokens(mc) if 'img' in MODES[mode] else 0
    return T, P, T + P


def _windows(mc, mode):
    T, P, N = _sizes(mc, mode)
    t = mc.max_text_len
    return [None, (0, 1), (t - 1, 3) if t + 2 <= N else (N - 3, 3)]


def _compare(got, want, L, N, what):
    assert got.dtype == torch.float32 and not got.requires_grad and got.grad_fn is None and got.shape == want.shape, (
        what, got.shape, want.shape)
    got = got.cpu().double()
    zero = want == 0
    assert (want >= 0).all() and (got[zero] == 0).all(), f'{what}: nonzero where fp64 is exactly 0'
    rel = ((got - want).abs()[~zero] / want[~zero]).max().item()
    bound = L * (N + 3) * 2.0 ** -23
    print(f'{what}: max relative error {rel:.3e} (bound {bound:.3e}); {int(zero.sum())} exact zeros of {want.numel()}, '
          f'nonzero values in [{want[~zero].min().item():.3e}, {want.max().item():.3e}]')
    assert rel <= bound, (what, rel, bound)


@pytest.mark.parametrize('method', ['gradcam', 'rollout'])
@pytest.mark.parametrize('mode', list(MODES))
def test_relevance_matches_fp64_reference(small, mode, method):
    module, mc, bd = small
    model = module.transformer
    T, P, N = _sizes(mc, mode)
    kw, score, L = _kw(mc, bd, mode), _score(mc), mc.depth
    alpha = attnmap.METHODS[method][0]
    if method == 'gradcam':
        maps = {'VLMO': model.attention_gradcam(score, kind='cam', head_mean=True, **kw),
                'VlmoModule': module.attention_gradcam(bd, infer_mode=mode, kind='cam', head_mean=True)}
    else:
        maps = {'VLMO': model.attention_maps(head_mean=True, **kw)}
        maps['VlmoModule'] = maps['VLMO']
    if mode == 'img-txt':
        assert isinstance(maps['VLMO'][0], dict) and not isinstance(maps['VLMO'][mc.fusion_layer], dict)
    for queries in _windows(mc, mode):
        for api in ('VLMO', 'VlmoModule'):
            cpu = {i: ({k: v.cpu() for k, v in m.items()} if isinstance(m, dict) else m.cpu()) for i, m in maps[api].items()}
            want = attnmap.relevance_reference(cpu, N, T or None, queries=queries, method=method, dtype=torch.float64)
            if api == 'VLMO':
                got = model.attention_relevance(score if method == 'gradcam' else None, queries=queries, method=method,
                                                **kw)
            else:
                got = module.attention_relevance(bd, infer_mode=mode, target='itm', queries=queries, method=method)
            nq = N if queries is None else queries[1]
            assert got.shape == (B, nq, N)
            _compare(got, want, L, N, f'{mode} {method} {api} queries={queries}')
    # the relevance is more than the identity part, and a padded text key's column is the identity part only
    full = model.attention_relevance(score, method=method, **kw).cpu()
    eye = torch.eye(N) * alpha ** L
    off = (full - eye).abs().amax(dim=(1, 2))
    print(f'{mode} {method}: max |R - alpha^L I| per sample {off.tolist()}')
    assert (off > 0).all()
    if T:
        pad = (bd['text_mask'] == 0).cpu()
        cols = full[:, :, :T].transpose(1, 2)[pad]                      # [padded keys, N]: the column of each
        rows = pad.nonzero()[:, 1]
        want_cols = torch.zeros_like(cols)
        want_cols[torch.arange(len(rows)), rows] = alpha ** L
        assert torch.equal(cols, want_cols)
    if mode == 'img-txt':
        grid = mc.img_size // mc.patch_size
        txt, img = attnmap.relevance_heatmaps(full, T, grid)
        assert txt.shape == (B, N, T) and img.shape == (B, N, grid, grid)
    if mode == 'txt_only':
        with pytest.raises(ValueError, match='queries'):
            model.attention_relevance(score, queries=(T - 1, 3), method=method, **kw)


def test_layer_subset_and_a_second_call(small):
    module, mc, bd = small
    model, kw, score = module.transformer, _kw(mc, bd, 'img-txt'), _score(mc)
    T, P, N = _sizes(mc, 'img-txt')
    sub = [0, mc.depth - 1]
    maps = model.attention_gradcam(score, layers=sub, kind='cam', head_mean=True, **kw)
    cpu = {i: ({k: v.cpu() for k, v in m.items()} if isinstance(m, dict) else m.cpu()) for i, m in maps.items()}
    want = attnmap.relevance_reference(cpu, N, T, queries=(0, 1), dtype=torch.float64)
    got = model.attention_relevance(score, layers=sub, queries=(0, 1), **kw)
    _compare(got, want, len(sub), N, f'layers={sub}')
    assert torch.equal(got, model.attention_relevance(score, layers=sub, queries=(0, 1), **kw))
    assert not torch.equal(got, model.attention_relevance(score, queries=(0, 1), **kw))
    roll = model.attention_relevance(layers=[1], queries=(0, 2), method='rollout', **kw)
    m1 = model.attention_maps(layers=[1], head_mean=True, **kw)[1]
    want = attnmap.relevance_reference({1: {k: v.cpu() for k, v in m1.items()}}, N, T, queries=(0, 2), method='rollout',
                                       dtype=torch.float64)
    _compare(roll, want, 1, N, 'rollout layers=[1]')


def test_no_side_effects(small):
    module, mc, bd = small
    model, kw, score = module.transformer, _kw(mc, bd, 'img-txt'), _score(mc)
    module.zero_grad(set_to_none=True)
    model.forward_features(**kw)[0].sum().backward()
    flags = {n: p.requires_grad for n, p in module.named_parameters()}
    held = {n: p.grad for n, p in module.named_parameters()}
    before = {n: g.clone() for n, g in held.items() if g is not None}
    assert before
    live = {m: model.attention_relevance(score, queries=(0, 1), method=m, **kw) for m in attnmap.METHODS}
    by_module = module.attention_relevance(bd, queries=(0, 1))
    assert not module.training and not model.training
    for n, p in module.named_parameters():
        assert p.requires_grad == flags[n], n
        assert p.grad is held[n], n
        if p.grad is not None:
            assert torch.equal(p.grad, before[n]), n
    try:
        for p in module.parameters():
            p.requires_grad_(False)
        frozen = {m: model.attention_relevance(score, queries=(0, 1), method=m, **kw) for m in attnmap.METHODS}
        frozen_module = module.attention_relevance(bd, queries=(0, 1))
    finally:
        for n, p in module.named_parameters():
            p.requires_grad_(flags[n])
    for m in attnmap.METHODS:
        assert torch.equal(frozen[m], live[m]), m
    assert torch.equal(frozen_module, by_module)
    module.zero_grad(set_to_none=True)


def test_refusals(small):
    from exploremultimodal_amd import engine
    module, mc, bd = small
    model, kw, score = module.transformer, _kw(mc, bd, 'img-txt'), _score(mc)
    T, P, N = _sizes(mc, 'img-txt')
    for obj, call in ((model, lambda **k: model.attention_relevance(score, **kw, **k)),
                      (module, lambda **k: module.attention_relevance(bd, **k))):
        for method in attnmap.METHODS:
            obj.train()
            try:
                with pytest.raises(RuntimeError, match='eval'):
                    call(method=method)
            finally:
                obj.eval()
        with pytest.raises(ValueError, match='method'):
            call(method='chefer')
        for bad in ((-1, 1), (0, 0), (N, 1), (N - 2, 3)):
            with pytest.raises(ValueError, match='queries'):
                call(queries=bad)
            with pytest.raises(ValueError, match='queries'):
                call(queries=bad, method='rollout')
        for bad in ([1, 0], [0, 0, 1], [2, 1, 0]):
            with pytest.raises(ValueError, match='layers'):
                call(layers=bad)
        with pytest.raises(ValueError, match='layers'):
            call(layers=[mc.depth])
        assert call(queries=(N - 1, 1)).shape == (B, 1, N)
    with pytest.raises(ValueError, match='score_fn'):
        model.attention_relevance(**kw)
    assert model.attention_relevance(method='rollout', queries=(0, 1), **kw).shape == (B, 1, N)   # no score_fn needed
    with pytest.raises(ValueError, match='scalar'):
        model.attention_relevance(lambda x, mask: x[:, 0].sum(-1), **kw)
    with pytest.raises(ValueError, match='target'):
        module.attention_relevance(bd, target='vqa')
    assert module.attention_relevance(bd, target='vqa', method='rollout', queries=(0, 1)).shape == (B, 1, N)

    class Sink:                                                 # any attached reducer: the call must not reach it
        def __getattr__(self, name):
            raise AssertionError(f'the gradient reducer was handed {name}')

    engine.GRAD_SINK = Sink()
    try:
        with pytest.raises(RuntimeError, match='reducer'):
            model.attention_relevance(score, **kw)
        with pytest.raises(RuntimeError, match='reducer'):
            module.attention_relevance(bd)
    finally:
        engine.GRAD_SINK = None
