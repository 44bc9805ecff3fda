"""VQAv2 fine-tuning on the host side (no GPU): the module builds with loss_names = ['vqa'] and phase = 'finetune_vqa'
with the reference's parameter names, the optimizer groups, checkpoint loading from a 224 px pretraining model, the
host-side target gate and the CPU path of compute_vqa against the reference formulas (objectives.py:12-21, 317-389)."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from exploremultimodal_amd import objectives, optim, synth
from exploremultimodal_amd.build import build_model


def _cfg(preset='mini', **over):
    return synth.make_config(preset, loss_names=['vqa'], phase='finetune_vqa', **over)


def test_vqa_module_builds_with_reference_names(golden_dir):
    cfg = _cfg(img_size=224)
    m = build_model(cfg)
    hs = cfg.model.embed_dim
    heads = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith('vqa_classifier.')}
    assert heads == {'vqa_classifier.0.weight': (2 * hs, hs), 'vqa_classifier.0.bias': (2 * hs,),
                     'vqa_classifier.1.weight': (2 * hs,), 'vqa_classifier.1.bias': (2 * hs,),
                     'vqa_classifier.3.weight': (3129, 2 * hs), 'vqa_classifier.3.bias': (3129,)}
    assert m.vqa_last is None
    assert m.vqa_classifier[1].eps == 1e-12
    assert isinstance(m.vqa_classifier[2], torch.nn.GELU) and m.vqa_classifier[2].approximate == 'none'
    # _init_weights: Linear biases zero, LayerNorm weight one
    assert not m.vqa_classifier[0].bias.detach().any() and not m.vqa_classifier[3].bias.detach().any()
    assert torch.equal(m.vqa_classifier[1].weight, torch.ones(2 * hs))
    # every parameter the reference run differentiated exists here under the same name
    g = np.load(os.path.join(golden_dir, 'vqa_mini.npz'))
    ref_names = {k[len('grad_norm.'):] for k in g.files if k.startswith('grad_norm.')}
    ours = {k for k, p in m.named_parameters() if p.requires_grad}
    assert ref_names <= ours, sorted(ref_names - ours)
    assert {k for k in ours if k.startswith('vqa_classifier.')} <= ref_names
    # _freeze_params (vlmo_module.py:165-167): no 'vl' expert below the fusion layer
    F_ = cfg.model.fusion_layer
    for i, b in enumerate(m.transformer.blocks):
        assert ('vl' in b.mlp) == (i >= F_), i
    # synthetic head weights carry the same keys and shapes
    sd = synth.synth_head_state_dict(cfg.model, 0, ['vqa'])
    assert {k: tuple(v.shape) for k, v in sd.items()} == heads


def test_vqa_refusals():
    cfg = _cfg()
    cfg.train.isda_lambda = 0.1
    with pytest.raises(NotImplementedError, match='isda'):
        build_model(cfg)
    for name in ('nlvr2', 'irtr', 'mpp', 'refcoco'):
        with pytest.raises(NotImplementedError):
            build_model(synth.make_config('mini', loss_names=['vqa', name], phase='finetune_vqa'))


def test_vqa_optimizer_groups():
    """finetune_vqa.yaml: lr_mult_head 50, lr_mult_fusion 5 (optim_factory.py:22-90)."""
    cfg = _cfg()
    m = build_model(cfg)
    base = 2e-5
    groups = optim.get_parameter_groups(m, base_lr=base, lr_mult_head=50, lr_mult_fusion=5, weight_decay=0.01,
                                        skip_list=m.no_weight_decay())
    lr_of = {id(p): gr['lr'] for gr in groups for p in gr['params']}
    F_, depth = cfg.model.fusion_layer, cfg.model.depth
    for k, p in m.named_parameters():
        if not p.requires_grad:
            continue
        if k.startswith('vqa_classifier.'):
            assert lr_of[id(p)] == pytest.approx(50 * base), k
        elif k.startswith('transformer.pooler') or any(k.startswith(f'transformer.blocks.{i}.') for i in range(F_, depth)):
            assert lr_of[id(p)] == pytest.approx(5 * base), k
        else:
            assert lr_of[id(p)] == pytest.approx(base), k
    tr = types.SimpleNamespace(opt=types.SimpleNamespace(name='adamw', eps=1e-8, betas=(0.9, 0.98), momentum=0.9),
                               weight_decay=0.01, base_lr=base, lr_mult_head=50, lr_mult_fusion=5)
    opt = optim.create_optimizer(tr, m)
    heads = [gr for gr in opt.param_groups if any(p is m.vqa_classifier[0].weight for p in gr['params'])]
    assert len(heads) == 1 and heads[0]['lr'] == pytest.approx(50 * base)
    fusion = [gr for gr in opt.param_groups if any(p is m.transformer.pooler.dense.weight for p in gr['params'])]
    assert len(fusion) == 1 and fusion[0]['lr'] == pytest.approx(5 * base)


def test_pretraining_checkpoint_loads_into_480px_vqa_model():
    """A 224 px pretraining state dict (pretrain_mum layout, pretraining heads) into a 480 px VQA module: the position
    table is resampled; only the VQA classifier is missing."""
    pre = build_model(synth.make_config('mini', loss_names=['itc', 'itm', 'mlm'], img_size=224))
    sd = {k: v.clone() for k, v in pre.state_dict().items()}
    vqa = build_model(_cfg(img_size=480))
    matching, is_beit = vqa.load_from_ckpt(sd)
    assert not is_beit
    assert sorted(matching.missing_keys) == sorted(k for k in vqa.state_dict() if k.startswith('vqa_classifier.'))
    assert vqa.transformer.pos_embed.shape[1] == (480 // 16) ** 2 + 1
    assert torch.equal(vqa.transformer.pos_embed[:, 0], pre.transformer.pos_embed[:, 0])


def test_attach_row_indices_records_the_target_gate():
    mc = _cfg().model
    b = synth.synth_batch(mc, 4, mim=False)
    b['vqa_targets'] = synth.synth_vqa_targets(4)
    objectives.attach_row_indices(b)
    assert b['_vqa_has_targets'] is True
    b = synth.synth_batch(mc, 4, mim=False)
    b['vqa_targets'] = torch.zeros(4, 3129)
    objectives.attach_row_indices(b)
    assert b['_vqa_has_targets'] is False
    b = synth.synth_batch(mc, 4, mim=False)
    objectives.attach_row_indices(b)
    assert '_vqa_has_targets' not in b


def test_synth_vqa_targets_and_unchanged_streams():
    y = synth.synth_vqa_targets(8, 3129, seed=5)
    assert y.shape == (8, 3129)
    n = (y > 0).sum(1)
    assert ((n[:-1] >= 1) & (n[:-1] <= 10)).all() and n[-1] == 0
    vals = torch.unique(y[y > 0])
    assert all(any(abs(v - t) < 1e-6 for t in (0.3, 0.6, 0.9, 1.0)) for v in vals.tolist())
    assert torch.equal(y, synth.synth_vqa_targets(8, 3129, seed=5))
    mc = synth.make_config('mini').model
    # the pretraining outputs of the head recipe keep their keys (a 'vqa' branch only adds keys)
    assert not any(k.startswith('vqa_') for k in synth.synth_head_state_dict(mc, 0))


def _cpu_model(kl_alpha=0.0, seed=3):
    cfg = _cfg()
    cfg.train.kl_alpha = kl_alpha
    m = build_model(cfg)
    m.load_state_dict(synth.synth_head_state_dict(cfg.model, 0, ['vqa']), strict=False)
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(5, cfg.model.embed_dim, generator=g)
    # the backbone is GPU-only: the CPU path of the head is checked on given pooled features
    m.infer = lambda batch, **kw: {'cls_feats': batch['_feats']}
    return m, feats


def _restated(m, feats, y):
    c = m.vqa_classifier
    h = F.gelu(F.layer_norm(F.linear(feats, c[0].weight, c[0].bias), (feats.shape[1] * 2,), c[1].weight, c[1].bias,
                            1e-12))
    logits = F.linear(h, c[3].weight, c[3].bias)
    loss = F.binary_cross_entropy_with_logits(logits, y) * y.shape[1]
    am = logits.argmax(1)
    score = y[torch.arange(len(am)), am].sum() / len(am)
    return logits, loss, score


def test_cpu_compute_vqa_matches_reference_formula():
    m, feats = _cpu_model()
    y = synth.synth_vqa_targets(5)
    with torch.no_grad():
        logits, loss, _ = _restated(m, feats, y)
    y[1, logits[1].argmax()] = 0.6            # a row whose arg-max is an answer
    ref_logits, ref_loss, ref_score = _restated(m, feats, y)
    ret = objectives.compute_vqa(m, {'_feats': feats, 'vqa_targets': y})
    assert set(ret) == {'vqa_logits', 'vqa_count', 'vqa_task_loss', 'vqa_targets', 'vqa_mean_score'}
    torch.testing.assert_close(ret['vqa_logits'], ref_logits)
    torch.testing.assert_close(ret['vqa_task_loss'], ref_loss)
    assert float(ret['vqa_mean_score']) == pytest.approx(float(ref_score)) and float(ref_score) == pytest.approx(0.6 / 5)
    assert ret['vqa_count'] == 5 and ret['vqa_targets'] is y
    s, c = objectives.compute_vqa_score(ref_logits, y)
    assert float(s) == pytest.approx(float(ref_score)) and c == 5
    # the host-side gate: same outputs without a device read; all-zero targets -> logits and count only
    ret2 = objectives.compute_vqa(m, {'_feats': feats, 'vqa_targets': y, '_vqa_has_targets': True})
    torch.testing.assert_close(ret2['vqa_task_loss'], ref_loss)
    for gate in (None, False):
        b = {'_feats': feats, 'vqa_targets': torch.zeros_like(y)}
        if gate is not None:
            b['_vqa_has_targets'] = gate
        assert set(objectives.compute_vqa(m, b)) == {'vqa_logits', 'vqa_count'}


def test_cpu_rdrop_kl_term():
    m, feats = _cpu_model(kl_alpha=1.0)
    y = synth.synth_vqa_targets(5)
    m.train()
    ret = objectives.compute_vqa(m, {'_feats': feats, 'vqa_targets': y})
    _, ref_loss, _ = _restated(m, feats, y)
    # same features twice (no dropout in the stand-in infer): the KL term vanishes, the loss is the single-pass loss
    assert abs(float(ret['vqa_kl_task_loss'])) < 1e-3
    torch.testing.assert_close(ret['vqa_task_loss'], ref_loss)
    m.eval()
    assert 'vqa_kl_task_loss' not in objectives.compute_vqa(m, {'_feats': feats, 'vqa_targets': y})
