"""VQAv2 fine-tuning through VlmoModule on the GPU: parity with the reference's own run of the same module
(tests/golden/vqa_mini{,_480}.npz, tools/gen_vqa_golden.py) at 224 and 480 px in training and eval mode, and the
training-step contracts: a prefetched batch without host synchronisation, autocast through the loss scaler, R-Drop,
merge_passes, and a short fine-tuning loop.  Tolerances as in test_module_gpu.py (bf16 backbone)."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import synth
from oracle.gen_golden import grad_probe

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASES = {'vqa_mini': dict(img_size=224), 'vqa_mini_480': dict(img_size=480, max_text_len=40)}


def _build(name='vqa_mini', **train):
    from exploremultimodal_amd.build import build_model
    cfg = synth.make_config('mini', loss_names=['vqa'], phase='finetune_vqa', **CASES[name])
    for k, v in train.items():
        setattr(cfg.train, k, v)
    mc = cfg.model
    model = build_model(cfg)
    sd = {'transformer.' + k: v for k, v in synth.synth_backbone_state_dict(mc, 0).items()}
    sd.update(synth.synth_head_state_dict(mc, 0, ['vqa']))
    r = model.load_state_dict(sd, strict=False)
    assert not r.unexpected_keys and not r.missing_keys, (r.unexpected_keys, r.missing_keys)
    return model.to(DEV), cfg


def _batch(cfg, g, device=DEV):
    B = int(g['meta.B'])
    b = synth.synth_batch(cfg.model, B, seed=1234, mim=False)
    b['vqa_targets'] = torch.from_numpy(g['vqa_targets'])
    return {k: v.to(device) for k, v in b.items()} if device else b


@pytest.mark.parametrize('train', [True, False])
@pytest.mark.parametrize('name', list(CASES))
def test_vqa_module_matches_reference(golden_dir, name, train):
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    model, cfg = _build(name)
    model.train(train)
    batch = _batch(cfg, g)
    B = int(g['meta.B'])
    ret = model(batch)
    assert set(ret) == {'vqa_logits', 'vqa_count', 'vqa_task_loss', 'vqa_targets', 'vqa_mean_score'}
    assert 'VQAHeadFn' in type(ret['vqa_task_loss'].grad_fn).__name__          # the HIP head, not torch ops
    assert ret['vqa_count'] == int(g['ret.vqa_count']) == B
    logits = ret['vqa_logits'].detach().float().cpu().numpy()
    err = np.abs(logits - g['ret.vqa_logits']).max()
    assert err <= 5e-2, err
    got, ref = float(ret['vqa_task_loss']), float(g['ret.vqa_task_loss'])
    assert abs(got - ref) <= 2e-2 + 2e-3 * abs(ref), (got, ref)
    # score: exact, unless a row's reference top-2 gap is a near-tie
    am = logits.argmax(1)
    ref_am = g['ret.vqa_logits'].argmax(1)
    tie = g['logits_top2_gap'] < 3e-2
    assert (am[~tie] == ref_am[~tie]).all()
    if not tie.any():
        assert float(ret['vqa_mean_score']) == pytest.approx(float(g['ret.vqa_mean_score']), abs=1e-6)
    ret['vqa_task_loss'].backward()
    fam_of = lambda k: re.sub(r'\.(v|l|vl)\.', '.X.', re.sub(r'blocks\.\d+\.', 'blocks.N.', k))
    fam = {}
    for k in (f[len('grad_norm.'):] for f in g.files if f.startswith('grad_norm.')):
        fam[fam_of(k)] = max(fam.get(fam_of(k), 0.0), float(g['grad_norm.' + k]))
    gmax = max(fam.values())
    rels, seen = [], 0
    for k, p in model.named_parameters():
        if 'grad_norm.' + k not in g.files:
            continue
        seen += 1
        assert p.grad is not None, k
        gr = p.grad.detach().float().cpu()
        gn = float(g['grad_norm.' + k])
        pr = (gr.double() * grad_probe(k, gr.shape).double()).sum().item()
        scale = max(gn, 0.05 * fam[fam_of(k)], 1e-3 * gmax) + 1e-12
        rels.append((max(abs(gr.norm().item() - gn), abs(pr - float(g['grad_probe.' + k]))) / scale, k))
    assert seen == sum(f.startswith('grad_norm.') for f in g.files)
    rels.sort(reverse=True)
    print('worst grads', [(round(r, 4), k) for r, k in rels[:6]])
    assert rels[0][0] <= 6e-2, rels[:6]


@pytest.mark.parametrize('name', list(CASES))
def test_vqa_eval_without_answers(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    model, cfg = _build(name)
    model.eval()
    batch = _batch(cfg, g)
    batch['vqa_targets'] = torch.zeros_like(batch['vqa_targets'])
    with torch.no_grad():
        ret = model(batch)
    assert sorted(ret) == sorted(str(k) for k in g['eval.keys']) == ['vqa_count', 'vqa_logits']
    err = np.abs(ret['vqa_logits'].float().cpu().numpy() - g['eval.vqa_logits']).max()
    assert err <= 5e-2, err


def test_vqa_prefetched_step_has_no_host_sync(golden_dir):
    from exploremultimodal_amd.objectives import attach_row_indices
    g = np.load(os.path.join(golden_dir, 'vqa_mini.npz'))
    model, cfg = _build()
    model.train()
    host = _batch(cfg, g, device=None)
    attach_row_indices(host)
    assert host['_vqa_has_targets'] is True
    batch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in host.items()}
    model(dict(batch))['vqa_task_loss'].backward()          # first call: allocations, weight shadows
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        ret = model(dict(batch))
        ret['vqa_task_loss'].backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.isfinite(ret['vqa_task_loss']).item()
    assert all(p.grad is not None for p in model.vqa_classifier.parameters())


@pytest.mark.parametrize('amp_dtype', [torch.bfloat16, torch.float16])
def test_vqa_autocast_step_through_the_scaler(golden_dir, amp_dtype):
    from exploremultimodal_amd import optim
    g = np.load(os.path.join(golden_dir, 'vqa_mini.npz'))
    model, cfg = _build()
    model.train()
    batch = _batch(cfg, g)
    with torch.autocast('cuda', dtype=amp_dtype):
        ret = model(batch)
    assert ret['vqa_logits'].dtype == amp_dtype and ret['vqa_task_loss'].dtype == torch.float32
    ref = float(g['ret.vqa_task_loss'])
    assert abs(float(ret['vqa_task_loss']) - ref) <= 3e-2 + 3e-3 * abs(ref)
    params = [p for p in model.parameters() if p.requires_grad]
    before = model.vqa_classifier[3].weight.detach().clone()
    opt = optim.FusedAdam([{'params': params, 'lr': 1e-4, 'weight_decay': 0.01}], betas=(0.9, 0.98), eps=1e-8)
    norm = optim.NativeScalerWithGradNormCount()(ret['vqa_task_loss'], opt, clip_grad=5.0, parameters=params,
                                                 update_grad=True)
    torch.cuda.synchronize()
    assert torch.isfinite(torch.as_tensor(norm)).all() and float(norm) > 0
    for k, p in model.named_parameters():
        if p.grad is not None:
            assert p.grad.dtype == p.dtype and torch.isfinite(p.grad).all(), k
    assert not torch.equal(before, model.vqa_classifier[3].weight.detach())


def test_vqa_rdrop(golden_dir):
    g = np.load(os.path.join(golden_dir, 'vqa_mini.npz'))
    model, cfg = _build()
    model.train()
    batch = _batch(cfg, g)
    base = model(dict(batch))
    cfg.train.kl_alpha = 1.0
    ret = model(dict(batch))
    # dropout 0: the two passes agree, so the KL term vanishes and the averaged loss is the single-pass loss
    assert abs(float(ret['vqa_kl_task_loss'])) <= 1e-3
    assert float(ret['vqa_task_loss']) == pytest.approx(float(base['vqa_task_loss']), rel=1e-6, abs=1e-4)
    (ret['vqa_task_loss'] + ret['vqa_kl_task_loss']).backward()
    assert torch.isfinite(model.vqa_classifier[0].weight.grad).all()
    # dropout 0.1: the second pass draws its own masks -> a positive, finite KL term
    cfg2 = synth.make_config('mini', loss_names=['vqa'], phase='finetune_vqa', drop_rate=0.1, attn_drop_rate=0.1,
                             **CASES['vqa_mini'])
    from exploremultimodal_amd.build import build_model
    m2 = build_model(cfg2)
    m2.load_state_dict(model.state_dict())
    m2 = m2.to(DEV).train()
    cfg2.train.kl_alpha = 1.0
    r2 = m2(dict(batch))
    kl = float(r2['vqa_kl_task_loss'])
    assert np.isfinite(kl) and kl > 0
    (r2['vqa_task_loss'] + r2['vqa_kl_task_loss']).backward()
    assert all(torch.isfinite(p.grad).all() for p in m2.vqa_classifier.parameters())


def test_vqa_loss_survives_merge_passes(golden_dir):
    g = np.load(os.path.join(golden_dir, 'vqa_mini.npz'))
    model, cfg = _build()
    model.train()
    batch = _batch(cfg, g)
    plain = model(dict(batch))
    cfg.train.merge_passes = True
    merged = model(dict(batch))
    assert set(merged) == set(plain)
    torch.testing.assert_close(merged['vqa_task_loss'].detach(), plain['vqa_task_loss'].detach(), rtol=1e-6, atol=1e-4)
    torch.testing.assert_close(merged['vqa_logits'].detach(), plain['vqa_logits'].detach(), rtol=1e-5, atol=1e-5)


def test_vqa_short_finetune_lowers_the_loss(golden_dir):
    from exploremultimodal_amd import optim
    g = np.load(os.path.join(golden_dir, 'vqa_mini.npz'))
    model, cfg = _build()
    model.train()
    batch = _batch(cfg, g)
    groups = optim.get_parameter_groups(model, base_lr=1e-4, lr_mult_head=50, lr_mult_fusion=5, weight_decay=0.01,
                                        skip_list=model.no_weight_decay())
    opt = optim.FusedAdam(groups, betas=(0.9, 0.98), eps=1e-8)
    scaler = optim.NativeScalerWithGradNormCount()
    losses = []
    for _ in range(6):
        opt.zero_grad(set_to_none=True)
        loss = model(dict(batch))['vqa_task_loss']
        losses.append(float(loss))
        scaler(loss, opt, clip_grad=5.0, parameters=[p for p in model.parameters() if p.requires_grad], update_grad=True)
    torch.cuda.synchronize()
    print('losses', losses)
    assert all(np.isfinite(losses)) and losses[-1] < 0.9 * losses[0]
