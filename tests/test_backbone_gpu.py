"""HIP backbone (exploremultimodal_amd.vlmo.VLMO through the C-ABI) against the
reference's own outputs/gradients (tests/golden, made by oracle/gen_golden.py).
Tolerance: bf16 GEMM operands (8-bit mantissa) + fp32 accumulation/residual stream vs
the fp32 CPU reference.  Final-LN outputs (unit scale): max error <= 2e-2 + 2e-2*|ref|
for the 2-3 layer shapes and <= 3e-2 + 2e-2*|ref| with mean error <= 4e-3 for the
12-layer Base shape (error grows ~sqrt(depth); the synthetic layer-scale of 0.5 is 5x
the real init, which makes this harsher than a real checkpoint); gradients <= 5 % of
the reference gradient norm."""
import os
from functools import partial

import numpy as np
import pytest
import torch

from oracle import synth
from oracle.gen_golden import grad_probe, out_weights

pytestmark = pytest.mark.gpu
DEV = 'cuda'


PLAIN = dict(qkv_bias=False, init_values=None)      # the reference's optional branches (vlmo.py:57-62, 185-192)
MLP6 = dict(mlp_ratio=6)                            # an FFN width other than 4 d


def build(preset, model_over=None, **over):
    from exploremultimodal_amd.vlmo import VLMO, LayerNorm
    mc = synth.make_config(preset, **(model_over or {})).model
    m = VLMO(img_size=mc.img_size, patch_size=mc.patch_size, in_chans=mc.in_chans, num_classes=mc.num_classes,
             embed_dim=mc.embed_dim, depth=mc.depth, num_heads=mc.num_heads, mlp_ratio=mc.mlp_ratio,
             qkv_bias=mc.qkv_bias, drop_rate=over.get('drop', 0.0), attn_drop_rate=over.get('drop', 0.0),
             drop_path_rate=over.get('drop_path', 0.0), norm_layer=partial(LayerNorm, eps=1e-12),
             init_values=mc.init_values, vocab_size=mc.vocab_size, max_text_len=mc.max_text_len,
             fusion_layer=mc.fusion_layer)
    sd = synth.synth_backbone_state_dict(mc, 0, [('v', 'l', 'vl')] * mc.depth)
    r = m.load_state_dict(sd, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    return m.to(DEV), mc


def modes(mc, batch, B):
    P = synth.num_img_tokens(mc)
    im = torch.ones(B, P, dtype=torch.int64, device=DEV)
    b = {k: v.to(DEV) for k, v in batch.items()}
    return {
        'vl': dict(img=b['image'], txt=b['text_ids'], img_attn_masks=im, txt_attn_masks=b['text_mask']),
        'v': dict(img=b['image'], img_attn_masks=im),
        'l': dict(txt=b['text_ids'], txt_attn_masks=b['text_mask']),
        'vl_mim': dict(img=b['image'], txt=b['text_ids'], img_attn_masks=im, txt_attn_masks=b['text_mask'],
                       bool_masked_pos=b['image_bool_masked_pos'].flatten(1)),
    }


@pytest.mark.parametrize('name,preset', [('backbone_mini', 'mini'), ('backbone_small', 'small'),
                                         ('backbone_base_b2', 'base'), ('backbone_large_b2', 'large'),
                                         ('backbone_mini_plain', 'mini'), ('backbone_mini_mlp6', 'mini')])
def test_forward_backward_matches_reference(golden_dir, name, preset):
    """backbone_mini_plain: qkv_bias=False and init_values=None (no q/v bias, no layer-scale parameters).
    backbone_mini_mlp6: mlp_ratio=6, an FFN of 768 columns at d = 128 -- the saved-activation slabs and the backward
    temporaries are sized by the FFN width, not by 4 d."""
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    B = int(g['meta.B'])
    model, mc = build(preset, PLAIN if name.endswith('_plain') else MLP6 if name.endswith('_mlp6') else None)
    if name.endswith('_plain'):
        assert not any('gamma_' in k or 'q_bias' in k or 'v_bias' in k for k in model.state_dict())
    if name.endswith('_mlp6'):
        assert model.blocks[0].mlp_hidden_dim == 6 * mc.embed_dim == 768
    model.eval()
    batch = synth.synth_batch(mc, B, seed=1234)
    report = []
    for mode, kw in modes(mc, batch, B).items():
        model.zero_grad(set_to_none=True)
        x, m = model.forward_features(**kw)
        xc = x.detach().float().cpu()
        if f'{mode}.out' in g:
            ref = torch.from_numpy(g[f'{mode}.out'])
            got = xc
        else:
            ref = torch.from_numpy(g[f'{mode}.out_rows'])
            got = xc[:, ::17]
        err = (got - ref).abs()
        report.append((mode, err.max().item(), err.mean().item()))
        # error grows ~sqrt(depth): 2-3 layers 2e-2, Base (12) 3e-2, Large (24 layers, conf/model/vlmo_large.yaml) 4.5e-2
        atol = 2e-2 if mc.depth <= 3 else (3e-2 if mc.depth <= 12 else 4.5e-2)
        mean_tol = 4e-3 if mc.depth <= 12 else 6e-3
        assert (err <= atol + 2e-2 * ref.abs()).all(), f'{name}/{mode}: max err {err.max().item():.4f}'
        assert err.mean().item() <= mean_tol, f'{name}/{mode}: mean err {err.mean().item():.5f}'
        np.testing.assert_array_equal(m.cpu().numpy(), g[f'{mode}.mask'])
        pooled = model.pooler(x.detach()).detach().float().cpu().numpy()
        np.testing.assert_allclose(pooled, g[f'{mode}.pooled'], atol=2e-2, rtol=2e-2)
        if f'{mode}.grad_norm.norm.weight' not in g:
            continue
        R = out_weights(mode, x.shape).to(DEV)
        (x * R).sum().backward()
        worst = (0.0, '')
        for k, p in model.named_parameters():
            key = f'{mode}.grad_norm.{k}'
            if key not in g:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, f'{k}: grad where reference has none'
                continue
            gn = float(g[key])
            assert p.grad is not None, f'{k}: missing grad'
            gr = p.grad.detach().float().cpu()
            if f'{mode}.grad.{k}' in g:
                rel = (gr - torch.from_numpy(g[f'{mode}.grad.{k}'])).norm().item() / (gn + 1e-12)
            else:
                pr = (gr.double() * grad_probe(k, gr.shape).double()).sum().item()
                rel = max(abs(gr.norm().item() - gn) / (gn + 1e-12),
                          abs(pr - float(g[f'{mode}.grad_probe.{k}'])) / (gn + 1e-12))
            if rel > worst[0]:
                worst = (rel, k)
            assert rel <= 5e-2, f'{name}/{mode}: grad of {k} off by {rel:.3f} of its norm'
        report.append((mode + '.grad', worst[0], worst[1]))
    print(report)


def test_forward_interval_and_block_api(golden_dir):
    g = np.load(os.path.join(golden_dir, 'backbone_mini.npz'))
    model, mc = build('mini')
    model.eval()
    batch = synth.synth_batch(mc, 3, seed=1234)
    with torch.no_grad():
        xi = model.forward_interval(x=batch['image'].to(DEV), attn_masks=None, route='v', need_embed=True,
                                    bool_masked_pos=batch['image_bool_masked_pos'].flatten(1).to(DEV),
                                    in_layer=0, out_layer=mc.fusion_layer, need_norm=True)
    err = (xi.cpu() - torch.from_numpy(g['interval_v.out'])).abs().max().item()
    assert err <= 2e-2, err
    with pytest.raises(AssertionError):
        model.forward_interval(x=batch['image'].to(DEV), attn_masks=None, route='x')
    # Block.forward keeps the reference signature (x, mask, route) -> (x, attn)
    x = torch.randn(2, 17, mc.embed_dim, device=DEV)
    with torch.no_grad():
        y, attn = model.blocks[0](x, mask=torch.ones(2, 17, dtype=torch.int64, device=DEV), route='v')
    assert y.shape == x.shape and attn is None
    from oracle import vlmo_oracle
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref = vlmo_oracle.block(sd, 0, x.cpu(), torch.ones(2, 17, dtype=torch.int64), 'v', mc.num_heads)
    assert (y.cpu() - ref).abs().max().item() <= 2e-2


def test_training_mode_dropout_is_unbiased_and_seeded():
    model, mc = build('mini', drop=0.1, drop_path=0.1)
    batch = synth.synth_batch(mc, 8, seed=5)
    kw = modes(mc, batch, 8)['vl']
    model.eval()
    with torch.no_grad():
        ref, _ = model.forward_features(**kw)
    model.train()
    torch.manual_seed(7)
    a, _ = model.forward_features(**kw)
    torch.manual_seed(7)
    b, _ = model.forward_features(**kw)
    assert torch.equal(a, b), 'same torch seed must give the same dropout masks'
    c, _ = model.forward_features(**kw)
    assert not torch.equal(a, c)
    assert torch.isfinite(a).all()
    (a.float() ** 2).mean().backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    assert (a - ref).abs().mean().item() < 0.5   # perturbed, not destroyed


@pytest.mark.parametrize('comm', ['torch', 'native'])
def test_grad_reducer_rccl_single_rank(comm):
    """The RCCL path (side stream, bf16 comm buffers, hooks fired from the autograd thread) at world
    size 1: averaged gradients == local gradients up to one bf16 rounding.  comm='native': the collectives go through
    the library's own communicator (vlmo_comm_*) instead of torch.distributed."""
    import torch.distributed as dist
    from exploremultimodal_amd.dp import GradReducer
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='29541')
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    red = None
    try:
        model, mc = build('mini')
        model.train()
        red = GradReducer(model, comm=comm)
        assert (red.native is not None) == (comm == 'native')
        batch = synth.synth_batch(mc, 4, seed=3)
        kw = modes(mc, batch, 4)['vl']
        x, _ = model.forward_features(**kw)
        loss = x.float().square().mean()
        loss.backward()
        want = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        for p in model.parameters():
            p.grad = None
        x, _ = model.forward_features(**kw)
        loss = x.float().square().mean()
        red.prepare(loss)
        loss.backward()
        red.finish()
        torch.cuda.synchronize()
        got = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
        assert set(got) == set(want)
        for n in want:
            assert torch.allclose(got[n], want[n], rtol=1e-2, atol=1e-2 * want[n].abs().max().item() + 1e-12), n
    finally:
        if red is not None:
            red.close()
        dist.destroy_process_group()


@pytest.mark.parametrize('B,T,fusion', [(1, 5, None), (2, 16, 1), (3, 9, 2), (2, 16, 0)])
def test_edge_shapes_and_fusion_layer_override_vs_oracle(B, T, fusion):
    """Ragged cases the reference accepts: batch 1, text shorter than max_text_len (vlmo.py:254 positions 0..T-1),
    the ``fusion_layer`` call argument (vlmo.py:399-400; 0 is falsy there and means the constructor's value),
    padded text keys.  Forward and every parameter gradient against the fp32 oracle; tolerance as in the golden
    tests (bf16 GEMM operands): 3e-2 absolute on outputs of O(1) magnitude, 6 % on gradient norms."""
    from oracle import vlmo_oracle
    model, mc = build('mini')
    model.eval()
    g = torch.Generator().manual_seed(B * 100 + T)
    img = torch.randn(B, 3, mc.img_size, mc.img_size, generator=g)
    ids = torch.randint(1000, mc.vocab_size, (B, T), generator=g)
    ids[:, 0] = 101
    tmask = torch.ones(B, T, dtype=torch.int64)
    if T > 4:
        tmask[-1, T - 2:] = 0
        ids[-1, T - 2:] = 0
    im = torch.ones(B, synth.num_img_tokens(mc), dtype=torch.int64)
    x, m = model.forward_features(img=img.to(DEV), txt=ids.to(DEV), img_attn_masks=im.to(DEV), txt_attn_masks=tmask.to(DEV),
                                  fusion_layer=fusion)
    R = torch.randn(x.shape, generator=g)
    (x * R.to(DEV)).sum().backward()
    sd = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}
    ref, mref = vlmo_oracle.forward_features(sd, mc, img=img, txt=ids, img_attn_masks=im, txt_attn_masks=tmask,
                                             fusion_layer=fusion)
    (ref * R).sum().backward()
    assert x.shape == ref.shape == (B, T + synth.num_img_tokens(mc), mc.embed_dim)
    assert torch.equal(m.cpu(), mref)
    assert (x.detach().cpu() - ref.detach()).abs().max().item() <= 3e-2
    worst = (0.0, '')
    for k, p in model.named_parameters():
        gr = sd[k].grad
        if gr is None or gr.abs().max() == 0:
            assert p.grad is None or p.grad.abs().max().item() <= 1e-6, k
            continue
        assert p.grad is not None, k
        rel = (p.grad.detach().cpu() - gr).norm().item() / (gr.norm().item() + 1e-12)
        worst = max(worst, (rel, k))
    assert worst[0] <= 6e-2, worst
    with pytest.raises(AssertionError):
        model.forward_features(img=img.to(DEV), txt=ids.to(DEV), img_attn_masks=im.to(DEV), txt_attn_masks=tmask.to(DEV),
                               fusion_layer=mc.depth + 1)


def _vl_step(model, kw, R, seed):
    for p in model.parameters():
        p.grad = None
    torch.manual_seed(seed)
    x, _ = model.forward_features(**kw)
    (x * R).sum().backward()
    torch.cuda.synchronize()
    return x.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('preset,B', [('small', 5), ('mini', 3)])
def test_native_stack_path_equals_per_block_path(preset, B):
    """engine.StackFn over the whole pass (ONE vlmo_stack_fwd / vlmo_stack_bwd call) against one StackFn call per
    block (engine.USE_STACK off), training mode with dropout and drop-path from the same seed.  A one-block stack has
    none of vlmo_stack_bwd's cross-block logic -- norm1's backward fused with the FFN residual-branch backward of the
    block below (ln_resid_seg_bwd), weight-gradient batches spanning blocks, rotation of the temporary sets -- so this
    checks that logic against a run without it.  The forward output is bit-identical (same kernels, same order); the
    activation-gradient chain is the same too, and both sides fold the same fp32 column partials (fc1 bias from the
    GELU-derivative epilogue, q / v bias from the attention backward), so what differs is only the summation order
    inside the weight gradients and column sums (fp32: 1e-4 of the gradient's largest element, every parameter)."""
    from exploremultimodal_amd import engine
    model, mc = build(preset, drop=0.1, drop_path=0.1)
    model.train()
    batch = synth.synth_batch(mc, B, seed=77)
    kw = modes(mc, batch, B)['vl']
    R = torch.randn(B, mc.max_text_len + synth.num_img_tokens(mc), mc.embed_dim, device=DEV)
    old = engine.USE_STACK
    try:
        engine.USE_STACK = True
        xs, gs = _vl_step(model, kw, R, 3)
        engine.USE_STACK = False
        xb, gb = _vl_step(model, kw, R, 3)
    finally:
        engine.USE_STACK = old
    assert torch.equal(xs, xb), (xs - xb).abs().max()
    assert set(gs) == set(gb)
    for n in gb:
        tol = 1e-4 * gb[n].abs().max().item() + 1e-9
        assert (gs[n] - gb[n]).abs().max().item() <= tol, (n, (gs[n] - gb[n]).abs().max().item(), tol)


def test_stack_bwd_refuses_a_short_column_workspace(monkeypatch):
    """A two-block stack (the smallest with a block below), described the way the engine does it except that every
    block's ws_bytes is one fold slot short of vlmo_stack_bwd_ws_bytes: vlmo_stack_bwd returns an argument error that
    names the bytes it needs, before it enqueues anything -- the backward temporaries and the dx buffers, which the
    first kernels of a chain write, still hold what was put there.  The same pass with the whole workspace runs."""
    from exploremultimodal_amd import engine, hip
    model, mc = build('mini')
    assert mc.depth == 2
    B = 2
    kw = modes(mc, synth.synth_batch(mc, B, seed=80), B)['vl']
    L = hip.lib()
    slot = L.vlmo_reduce_ws_bytes(2 * mc.embed_dim)
    wire, seen = engine._wire_temporaries, {}

    def short_wire(D, k, nb, M, d, hid, sc, dxo, dx_in):
        wire(D, k, nb, M, d, hid, sc, dxo, dx_in)
        nseq = sum(D.nseq[a] for a in range(D.n_attn))
        assert D.ws_bytes == L.vlmo_stack_bwd_ws_bytes(D.M, D.d, D.hidden, 2 * B)
        seen.setdefault('need', []).append(L.vlmo_stack_bwd_ws_bytes(D.M, D.d, D.hidden, nseq))
        D.ws_bytes -= slot
        if k == 0:
            seen['bufs'] = [sc.tb, sc.dxs, dx_in]
            for t in seen['bufs']:
                t.fill_(3.0)
    monkeypatch.setattr(engine, '_wire_temporaries', short_wire)
    x, _ = model.forward_features(**kw)
    with pytest.raises(RuntimeError) as e:
        x.sum().backward()
    torch.cuda.synchronize()
    assert len(seen['need']) == 2
    assert 'vlmo_stack_bwd' in str(e.value) and 'rc=-1' in str(e.value), str(e.value)
    assert f'need {seen["need"][-1]} bytes' in str(e.value), str(e.value)       # block 0 is checked first
    for t in seen['bufs']:
        assert bool((t == 3.0).all())
    monkeypatch.setattr(engine, '_wire_temporaries', wire)
    for p in model.parameters():
        p.grad = None
    x, _ = model.forward_features(**kw)
    x.sum().backward()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


@pytest.mark.parametrize('stack', [True, False])
def test_one_stream_and_side_stream_schedules_give_the_same_gradients(stack):
    """engine.OVERLAP_WGRAD: weight gradients and column folds on the caller's stream (the default without a gradient
    reducer) or on the side stream (the default under one, VLMO_OVERLAP_WGRAD=1 always).  Same kernels on the same
    operands: outputs bit-identical, gradients equal up to the order of the fp32 atomics (column folds, embeddings).
    stack: one engine.StackFn call per pass, or one per block (engine.USE_STACK off)."""
    from exploremultimodal_amd import engine
    model, mc = build('small', drop=0.1, drop_path=0.1)
    model.train()
    B = 5
    batch = synth.synth_batch(mc, B, seed=79)
    kw = modes(mc, batch, B)['vl']
    R = torch.randn(B, mc.max_text_len + synth.num_img_tokens(mc), mc.embed_dim, device=DEV)
    old = engine.USE_STACK, engine.OVERLAP_WGRAD
    try:
        engine.USE_STACK = stack
        engine.OVERLAP_WGRAD = False
        x1, g1 = _vl_step(model, kw, R, 3)
        engine.OVERLAP_WGRAD = True
        x2, g2 = _vl_step(model, kw, R, 3)
        engine.OVERLAP_WGRAD = None
        x3, g3 = _vl_step(model, kw, R, 3)          # auto: no reducer here -> one stream
    finally:
        engine.USE_STACK, engine.OVERLAP_WGRAD = old
    assert torch.equal(x1, x2) and torch.equal(x1, x3)
    assert set(g1) == set(g2) == set(g3)
    for n in g1:
        tol = 1e-3 * g1[n].abs().max().item() + 1e-9        # the bound two runs of ONE schedule are held to above
        assert (g1[n] - g2[n]).abs().max().item() <= tol, (n, (g1[n] - g2[n]).abs().max().item(), tol)
        assert (g1[n] - g3[n]).abs().max().item() <= tol, (n, (g1[n] - g3[n]).abs().max().item(), tol)


@pytest.mark.parametrize('stack', [True, False])
def test_split_backward_attention_regenerates_the_forward_dropout_mask(stack):
    """Below the fusion layer text and image sequences share ONE forward attention launch and the backward runs as two
    right-sized launches (engine._split_backward_attention).  With attention dropout on (vlmo.py:93; 0.1 in every
    reference config) the text launch must regenerate the mask of ITS sequences of the shared forward launch
    (VlmoBlockDesc.attn_seq0 / attn_seed_idx): gradients with the split on and off agree to summation-order
    rounding.  (Round 3 shipped the split with the text launch keyed as a second launch: a different mask.)
    stack: one engine.StackFn call per pass, or one per block (engine.USE_STACK off)."""
    from exploremultimodal_amd import engine
    model, mc = build('small', drop=0.1)
    model.train()
    B = 5
    batch = synth.synth_batch(mc, B, seed=78)
    kw = modes(mc, batch, B)['vl']
    R = torch.randn(B, mc.max_text_len + synth.num_img_tokens(mc), mc.embed_dim, device=DEV)
    old = engine.USE_STACK, engine.SPLIT_BWD_ATTENTION
    try:
        engine.USE_STACK = stack
        engine.SPLIT_BWD_ATTENTION = True
        xs, gs = _vl_step(model, kw, R, 3)
        engine.SPLIT_BWD_ATTENTION = False
        xb, gb = _vl_step(model, kw, R, 3)
    finally:
        engine.USE_STACK, engine.SPLIT_BWD_ATTENTION = old
    assert torch.equal(xs, xb)
    assert set(gs) == set(gb)
    for n in gb:
        tol = 1e-3 * gb[n].abs().max().item() + 1e-9
        assert (gs[n] - gb[n]).abs().max().item() <= tol, (n, (gs[n] - gb[n]).abs().max().item(), tol)


@pytest.mark.parametrize('preset,B,out_tol,mean_tol,grad_tol', [('base', 64, 3e-2, 4e-3, 5e-2),
                                                                ('large', 32, 4.5e-2, 6e-3, 8e-2)])
def test_full_batch_against_oracle(preset, B, out_tol, mean_tol, grad_tol):
    """BASELINE.json configs[1] at its FULL size -- VLMo-Base, 64 pairs, 224x224 image + 64-token text (M = 16 704
    packed rows), dropout 0 -- forward + backward through the HIP path against the fp32 CPU oracle on identical
    weights and inputs.  This is the only test in which the 256x256 ping-pong NT kernels, the grouped expert
    launches, the batched no-split weight-gradient launches and the side-stream deferral run in situ at the
    benchmark's shapes.  Tolerance: the bound of the Base golden test (3e-2 + 2e-2 |ref| on the final-LN output) for all but 1e-5 of the
    12.8 M elements and twice that bound for every element, mean error
    <= 4e-3; every parameter gradient within 5 % of its norm).  Second case: the per-GPU workload of BASELINE.json
    configs[3] -- VLMo-Large, 32 pairs (M = 8 352): the shapes at which the 192x256 tile is picked; tolerances of the
    Large golden test (24 layers)."""
    from oracle import vlmo_oracle
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    model, mc = build(preset)
    for b in model.blocks[:mc.fusion_layer]:       # pretrain_mum layout (vlmo_module.py:165-167)
        del b.mlp['vl']
    model.eval()
    batch = synth.synth_batch(mc, B, seed=1234)
    kw = modes(mc, batch, B)['vl']
    x, m = model.forward_features(**kw)
    g = torch.Generator().manual_seed(9)
    R = torch.randn(x.shape, generator=g) / 64.0
    (x * R.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}
    im = torch.ones(B, synth.num_img_tokens(mc), dtype=torch.int64)
    ref, mref = vlmo_oracle.forward_features(sd, mc, img=batch['image'], txt=batch['text_ids'], img_attn_masks=im,
                                             txt_attn_masks=batch['text_mask'])
    (ref * R).sum().backward()
    assert torch.equal(m.cpu(), mref)
    err = (x.detach().cpu() - ref.detach()).abs()
    # 12.8 M outputs of 12 (24) bf16 layers: the bound of the small golden tests holds for all but a 1e-5 fraction of the
    # elements (which ones exceed it moves with the summation order of any kernel on the path), twice the bound for all
    bound = out_tol + 2e-2 * ref.detach().abs()
    over = (err > bound).float().mean().item()
    assert over <= 1e-5, (over, err.max().item())
    assert (err <= 2 * bound).all(), err.max().item()
    assert err.mean().item() <= mean_tol, err.mean().item()
    worst = (0.0, '')
    for k, p in model.named_parameters():
        gr = sd[k].grad
        if gr is None or gr.abs().max() == 0:
            assert p.grad is None or p.grad.abs().max().item() <= 1e-6, k
            continue
        assert p.grad is not None, k
        rel = (p.grad.detach().cpu() - gr).norm().item() / (gr.norm().item() + 1e-12)
        worst = max(worst, (rel, k))
        assert rel <= grad_tol, (k, rel)
    print(f'{preset} B={B}: ' + 'max err %.4f mean %.5f worst grad %.4f (%s)' % (err.max().item(), err.mean().item(), *worst))
    # ---- the sharper instrument.  Element-wise bounds cannot be pulled in: bf16 rounding is CHAOTIC across layers (a 1e-7
    # summation-order difference in front of a rounding flips 1e-7 / ulp of the elements by a whole ulp, three roundings later
    # the two computations round independently), so even the restatement with ITS operands rounded to bf16 at the engine's
    # rounding points (oracle.vlmo_oracle.bf16_operands) stays ~2e-3 rms from the engine (measured round 4: mean |err| 0.0018
    # against 0.0025 for the fp32 restatement, same maximum).  What that oracle does remove is the SYSTEMATIC part of the
    # rounding (weights and activations rounded the same way on both sides), so the error against it must be pure noise:
    # zero mean overall and per output column, no token row that stands out, unit regression slope.  12.8 M elements make
    # these averages sharp to 1e-5 .. 1e-4 -- two orders under the element bound: a mis-added bias, a wrong scale, a
    # mis-keyed mask or a dropped tile row shows here long before it moves the maximum.
    sd2 = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}
    with vlmo_oracle.bf16_operands():
        ref2, _ = vlmo_oracle.forward_features(sd2, mc, img=batch['image'], txt=batch['text_ids'], img_attn_masks=im,
                                               txt_attn_masks=batch['text_mask'])
        (ref2 * R).sum().backward()
    r2 = ref2.detach()
    e2 = x.detach().cpu() - r2                                   # signed
    valid = mref.bool().unsqueeze(-1) if mref is not None else torch.ones_like(e2[..., :1], dtype=torch.bool)
    e2v = e2[valid.expand_as(e2)].view(-1, e2.shape[-1])           # rows of real (unpadded) tokens
    r2v = r2[valid.expand_as(r2)].view(-1, r2.shape[-1])
    rms = e2v.square().mean().sqrt().item()
    gmean = e2v.mean().item()
    col = e2v.mean(0).abs().max().item()
    row_rms = e2v.square().mean(1).sqrt()
    slope = ((x.detach().cpu()[valid.expand_as(e2)].view(-1, e2.shape[-1]) * r2v).sum() / r2v.square().sum()).item() - 1.0
    print(f'{preset} B={B} vs bf16-operand oracle: max |err| %.5f mean |err| %.6f rms %.6f | global mean %.2e  worst column mean %.2e  '
          f'worst row rms / rms %.2f  slope - 1 %.2e' % (e2.abs().max().item(), e2.abs().mean().item(), rms, gmean, col,
                                                         (row_rms.max() / rms).item(), slope))
    depth_f = 1.0 if preset == 'base' else 1.5
    assert rms <= 3.5e-3 * depth_f, rms
    assert abs(gmean) <= 5e-6 * depth_f, gmean           # measured round 4: 4e-8 (Base), 3e-8 (Large)
    assert col <= 3e-4 * depth_f, col                    # 7e-5, 1.9e-4
    assert (row_rms.max() / rms).item() <= 5.0, (row_rms.max() / rms).item()     # 2.7, 2.3
    assert abs(slope) <= 5e-5 * depth_f, slope           # 3e-6, 6e-6
    worst2 = (0.0, '')
    for k, p in model.named_parameters():
        gr = sd2[k].grad
        if gr is None or gr.abs().max() == 0:
            continue
        rel = (p.grad.detach().cpu() - gr).norm().item() / (gr.norm().item() + 1e-12)
        worst2 = max(worst2, (rel, k))
    print('worst grad vs bf16-operand oracle %.4f (%s)' % worst2)
    assert worst2[0] <= (1.5e-2 if preset == 'base' else 2e-2), worst2      # 0.8 %, 1.1 %


def test_second_backward_accumulates_in_place():
    """A second backward() over parameters that already hold the engine's gradient views (a gradient-accumulation
    micro-step; multimodal.py:260,316-323) adds into them inside the weight-gradient kernels when the loop opts in with
    engine.accumulate_into_grad() (the package's NativeScalerWithGradNormCount does): same storage afterwards,
    values = sum of the two passes.  Decided per parameter GROUP: an image-only pass after a VL pass reuses the shared
    groups and the image experts it already fed and hands autograd fresh tensors only for experts seen the first time."""
    from exploremultimodal_amd import engine
    model, mc = build('mini')
    model.eval()
    batch = synth.synth_batch(mc, 3, seed=5)
    kw = modes(mc, batch, 3)
    blk = [p for n, p in model.named_parameters() if 'blocks.' in n]

    def run(mode, scale):
        x, _ = model.forward_features(**kw[mode])
        with engine.accumulate_into_grad():
            (x.float().square().mean() * scale).backward()

    run('vl', 1.0)
    torch.cuda.synchronize()
    first = {id(p): (p.grad.data_ptr(), p.grad.clone()) for p in blk if p.grad is not None}
    assert first
    run('vl', 2.0)          # same pass again, twice the loss: every gradient must become 3x the first one
    torch.cuda.synchronize()
    for p in blk:
        if p.grad is None:
            continue
        ptr, g1 = first[id(p)]
        assert p.grad.data_ptr() == ptr                         # accumulated in place, not replaced by autograd's sum
        ref = 3.0 * g1
        assert torch.allclose(p.grad, ref, rtol=2e-2, atol=2e-2 * ref.abs().max().item() + 1e-12)
    # an image-only pass touches the image experts and the shared parameters only: text-expert gradients stay as they are,
    # and every group that already had a gradient keeps its storage (per-group reuse)
    before = {id(p): (p.grad.data_ptr(), p.grad.clone()) for p in blk if p.grad is not None}
    run('v', 1.0)
    torch.cuda.synchronize()
    changed = sum(int(not torch.equal(p.grad, before[id(p)][1])) for p in blk if id(p) in before)
    assert 0 < changed < len(before)      # (the image experts of the fusion layers get their first gradient here)
    assert all(p.grad.data_ptr() == before[id(p)][0] for p in blk if id(p) in before)
    # without the opt-in a further backward() leaves the accumulation to autograd: values still add up
    snap = {id(p): p.grad.clone() for p in blk if p.grad is not None}
    x, _ = model.forward_features(**kw['v'])
    x.float().square().mean().backward()
    torch.cuda.synchronize()
    moved = sum(int(not torch.equal(p.grad, snap[id(p)])) for p in blk if id(p) in snap)
    assert moved > 0


def _three_pass_loss(model, kw):
    xv, _ = model.forward_features(**kw['v'])
    xl, _ = model.forward_features(**kw['l'])
    xvl, _ = model.forward_features(**kw['vl'])
    return xv.float().square().mean() + 2.0 * xl.float().square().mean() + 3.0 * xvl.float().square().mean()


def test_passes_of_one_walked_backward_accumulate_in_place():
    """V -> L -> VL passes of ONE step (the merged four-objective step, objectives.py:40-314) summed into one loss and
    ONE backward() inside engine.inplace_passes(loss): the graph walk finds no producer but StackFn nodes for any block
    parameter group, so the first StackFn node that reaches a group returns its gradient buffer, the later nodes of the
    same graph task add into it inside the weight-gradient kernels and return nothing (engine._task_flats), and autograd
    has nothing to add.  Gradients equal those of the unfused path (VLMO_INPLACE_ACCUM off: one fresh tensor per pass,
    summed by autograd) to summation-order rounding -- under backward() AND under autograd.grad(), which must not touch
    .grad at all -- and so do those of a plain backward() / autograd.grad() outside the walk (fresh gradients)."""
    from exploremultimodal_amd import engine
    model, mc = build('mini')
    model.eval()
    batch = synth.synth_batch(mc, 3, seed=6)
    kw = modes(mc, batch, 3)
    names = [n for n, p in model.named_parameters() if 'blocks.' in n]
    blk = [p for n, p in model.named_parameters() if 'blocks.' in n]

    def grads(inplace, use_grad_api, walked=True):
        old = engine.INPLACE_ACCUM
        engine.INPLACE_ACCUM = inplace
        try:
            for p in model.parameters():
                p.grad = None
            loss = _three_pass_loss(model, kw)
            with engine.inplace_passes(loss, enabled=walked):
                if use_grad_api:
                    used = [p for p in blk]
                    out = torch.autograd.grad(loss, used, allow_unused=True)
                    assert all(p.grad is None for p in model.parameters())         # autograd.grad leaves .grad alone
                    res = {n: g.clone() for n, g in zip(names, out) if g is not None}
                else:
                    loss.backward()
                    res = {n: p.grad.clone() for n, p in zip(names, blk) if p.grad is not None}
                if inplace and walked:
                    # the in-place path really ran: every group the walk permitted (here: all of them) got ONE buffer,
                    # which the second and third pass found
                    assert engine._TASK_FLATS['groups'], 'the walk permitted no group of an engine-only loss'
                    assert set(engine._TASK_FLATS['flats']) == set(engine._TASK_FLATS['groups'])
            torch.cuda.synchronize()
            return res
        finally:
            engine.INPLACE_ACCUM = old

    ref = grads(False, False)
    for api in (False, True):
        for walked in (True, False):
            got = grads(True, api, walked)
            assert set(got) == set(ref)
            for n in ref:
                tol = 2e-3 * ref[n].abs().max().item() + 1e-9
                assert (got[n] - ref[n]).abs().max().item() <= tol, (api, walked, n, (got[n] - ref[n]).abs().max().item(), tol)


def test_backward_after_a_parameter_update_is_refused_like_stock_autograd():
    """forward A, in-place parameter update, forward B (ShadowCache.refresh re-casts the stale bf16 shadows), backward A: stock
    autograd refuses this (a tensor saved for backward was modified), and so does the engine -- StackFn saves the
    parameters themselves, so the version check fires before any kernel could read a refreshed shadow (ADVICE r03 asked
    what happens here; the refresh additionally leaves a shadow pair that a live graph still holds untouched)."""
    model, mc = build('mini')
    model.eval()
    batch = synth.synth_batch(mc, 3, seed=5)
    kw = modes(mc, batch, 3)['vl']
    xa, _ = model.forward_features(**kw)
    saved = {n: p.detach().clone() for n, p in model.named_parameters()}
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() == 2 and 'blocks.' in n:
                p.mul_(1.5)                             # bumps the version counter: every block shadow is stale
    xb, _ = model.forward_features(**kw)
    assert not torch.equal(xa, xb)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        xa.sum().backward()
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(saved[n])
    for p in model.parameters():
        p.grad = None
    xc, _ = model.forward_features(**kw)                # the engine is usable afterwards
    xc.sum().backward()
    assert torch.allclose(xc, xa)
