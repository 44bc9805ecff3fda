"""VQAv2 fine-tuning with ISDA on the host side (no GPU): the module layout and refusals, the optimizer group of
vqa_last, checkpoints, and the CPU path of compute_vqa against the reference's own three-step run
(tests/golden/vqa_isda_mini.npz, tools/gen_isda_golden.py) at fp32 tolerance."""
import os
import types

import numpy as np
import pytest
import torch

from exploremultimodal_amd import checkpoint, objectives, optim, synth
from exploremultimodal_amd.build import build_model
from oracle.gen_golden import grad_probe

EST = ('isda_head.estimator.count', 'isda_head.estimator.mean', 'isda_head.estimator.cov')


def _cfg(**train):
    cfg = synth.make_config('mini', loss_names=['vqa'], phase='finetune_vqa', img_size=224)
    for k, v in dict(dict(isda_lambda=7.5, epochs=2, cur_epoch=1), **train).items():
        setattr(cfg.train, k, v)
    return cfg


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'vqa_isda_mini.npz'))


def _model(**train):
    cfg = _cfg(**train)
    m = build_model(cfg)
    A = 2 * cfg.model.embed_dim
    sd = dict(synth.synth_isda_head_state_dict(cfg.model, 0))
    sd.update(synth.synth_isda_estimator(A, 3129, 0))
    r = m.load_state_dict(sd, strict=False)
    assert not r.unexpected_keys and all(k.startswith('transformer.') for k in r.missing_keys)
    m.infer = lambda batch, **kw: {'cls_feats': batch['_feats']}        # the CPU path of the head on given features
    return m, cfg


def test_isda_module_layout(golden):
    m, cfg = _model()
    hs = cfg.model.embed_dim
    assert list(m.state_dict().keys()) == list(golden['keys'])
    assert len(m.vqa_classifier) == 3
    assert isinstance(m.vqa_classifier[2], torch.nn.GELU) and m.vqa_classifier[1].eps == 1e-12
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith('transformer.')}
    assert shapes == {'vqa_classifier.0.weight': (2 * hs, hs), 'vqa_classifier.0.bias': (2 * hs,),
                      'vqa_classifier.1.weight': (2 * hs,), 'vqa_classifier.1.bias': (2 * hs,),
                      'vqa_last.weight': (3129, 2 * hs), 'vqa_last.bias': (3129,),
                      EST[0]: (3129,), EST[1]: (3129, 2 * hs), EST[2]: (3129, 2 * hs)}
    fresh = build_model(_cfg())
    assert not fresh.vqa_last.bias.detach().any() and not fresh.vqa_classifier[0].bias.detach().any()
    assert torch.equal(fresh.vqa_classifier[1].weight, torch.ones(2 * hs))
    for k in EST:
        t = fresh.state_dict()[k]
        assert t.dtype == torch.float32 and not t.any()
    assert {k for k, _ in fresh.named_buffers() if k.startswith('isda_head.')} == set(EST)


def test_isda_refusals():
    with pytest.raises(NotImplementedError, match='R-Drop'):
        build_model(_cfg(kl_alpha=1.0))
    for drop in ('epochs', 'cur_epoch'):
        cfg = _cfg()
        delattr(cfg.train, drop)
        with pytest.raises(NotImplementedError, match=r'isda_lambda.*epochs.*cur_epoch'):
            build_model(cfg)
    plain = synth.make_config('mini', loss_names=['vqa'], phase='finetune_vqa')
    assert not hasattr(plain.train, 'epochs') and not hasattr(plain.train, 'cur_epoch')


def test_isda_vqa_last_in_head_group():
    m, _ = _model()
    base = 2e-5
    groups = optim.get_parameter_groups(m, base_lr=base, lr_mult_head=50, lr_mult_fusion=5, weight_decay=0.01,
                                        skip_list=m.no_weight_decay())
    lr_of = {id(p): gr['lr'] for gr in groups for p in gr['params']}
    for p in (m.vqa_last.weight, m.vqa_last.bias, m.vqa_classifier[0].weight):
        assert lr_of[id(p)] == pytest.approx(50 * base)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def test_isda_cpu_path_matches_reference(golden):
    m, cfg = _model()
    m.train()
    est = m.isda_head.estimator
    for s in range(3):
        p = f's{s}.'
        feats = torch.from_numpy(golden[p + 'cls_feats'])
        y = torch.from_numpy(golden[p + 'vqa_targets'])
        m.zero_grad(set_to_none=True)
        ret = objectives.compute_vqa(m, {'_feats': feats, 'vqa_targets': y})
        assert set(ret) == {'vqa_logits', 'vqa_count', 'vqa_task_loss', 'vqa_targets', 'vqa_mean_score'}
        logits = ret['vqa_logits'].detach().numpy()
        assert _rel(logits, golden[p + 'ret.vqa_logits']) < 1e-5, s
        # the augmentation on its own (the logits bound could hide it)
        aug_ref = golden[p + 'ret.vqa_logits'] - golden[p + 'z']
        assert np.abs(aug_ref).max() > 0.1
        plain = m.vqa_last(m.vqa_classifier(feats)).detach().numpy()
        assert _rel(logits - plain, aug_ref) < 1e-4, s
        assert float(ret['vqa_task_loss']) == pytest.approx(float(golden[p + 'ret.vqa_task_loss']), rel=1e-5)
        assert float(ret['vqa_mean_score']) == pytest.approx(float(golden[p + 'ret.vqa_mean_score']), abs=1e-6)
        touched = torch.from_numpy(golden[p + 'touched'])
        assert torch.equal(est.count, torch.from_numpy(golden[p + 'count']))
        assert _rel(est.mean[touched].numpy(), golden[p + 'mean_rows']) < 1e-5
        assert _rel(est.cov[touched].numpy(), golden[p + 'cov_rows']) < 1e-5
        ret['vqa_task_loss'].backward()
        rows = torch.from_numpy(golden[p + 'grad_rows_idx'])
        assert _rel(m.vqa_last.weight.grad[rows].numpy(), golden[p + 'grad_rows']) < 1e-4, s
        for name, prm in m.named_parameters():
            key = p + 'grad_norm.' + name
            if key not in golden.files or not name.startswith('vqa_'):      # the backbone does not run on the CPU
                continue
            g = prm.grad.detach().double()
            assert float(g.norm()) == pytest.approx(float(golden[key]), rel=1e-4), name
            probe = float((g * grad_probe(name, g.shape).double()).sum())
            assert probe == pytest.approx(float(golden[p + 'grad_probe.' + name]), rel=1e-3, abs=1e-6 * float(golden[key])), name


def test_isda_eval_mode_leaves_buffers(golden):
    m, _ = _model()
    before = {k: v.clone() for k, v in m.state_dict().items() if k in EST}
    feats = torch.from_numpy(golden['s0.cls_feats'])
    y = torch.from_numpy(golden['s0.vqa_targets'])
    m.eval()
    with torch.no_grad():
        ret = objectives.compute_vqa(m, {'_feats': feats, 'vqa_targets': y})
    assert _rel(ret['vqa_logits'].numpy(), golden['s0.z']) < 1e-5
    m.train()
    with torch.no_grad():           # training mode without answers: no update either
        ret = objectives.compute_vqa(m, {'_feats': feats, 'vqa_targets': torch.zeros_like(y)})
    assert set(ret) == {'vqa_logits', 'vqa_count'}
    for k, v in m.state_dict().items():
        if k in EST:
            assert torch.equal(v, before[k]), k


def test_isda_estimator_survives_checkpoint(tmp_path, golden):
    m, cfg = _model()
    m.train()
    objectives.compute_vqa(m, {'_feats': torch.from_numpy(golden['s0.cls_feats']),
                               'vqa_targets': torch.from_numpy(golden['s0.vqa_targets'])})
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-4)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 1.0)
    scaler = torch.amp.GradScaler('cuda', enabled=False)
    run = types.SimpleNamespace(output_dir=str(tmp_path))
    name = checkpoint.save_model(run, 0, m, m, opt, sched, scaler)
    state = torch.load(os.path.join(tmp_path, name), map_location='cpu', weights_only=False)
    m2, _ = _model()
    m2.load_state_dict(state['model'])
    for k in EST:
        assert torch.equal(m2.state_dict()[k], m.state_dict()[k]), k
    assert not torch.equal(m.state_dict()[EST[0]], synth.synth_isda_estimator(256, 3129, 0)[EST[0]])


def test_pretraining_checkpoint_loads_into_isda_model():
    pre = build_model(synth.make_config('mini', loss_names=['itc', 'itm', 'mlm'], img_size=224))
    sd = {k: v.clone() for k, v in pre.state_dict().items()}
    m = build_model(_cfg())
    matching, is_beit = m.load_from_ckpt(sd)
    assert not is_beit
    want = [k for k in m.state_dict() if k.startswith(('vqa_classifier.', 'vqa_last.', 'isda_head.'))]
    assert sorted(matching.missing_keys) == sorted(want)
    assert set(EST) <= set(want) and 'vqa_last.weight' in want


def test_synth_isda_inputs():
    mc = synth.make_config('mini').model
    sd = synth.synth_isda_head_state_dict(mc, 0)
    ref = synth.synth_head_state_dict(mc, 0, ['vqa'])
    assert torch.equal(sd['vqa_last.weight'], ref['vqa_classifier.3.weight'])
    assert not any(k.startswith('vqa_classifier.3') for k in sd)
    est = synth.synth_isda_estimator(256, 3129, 0)
    c = est[EST[0]]
    assert (c[0::2] == 0).all() and ((c[1::2] >= 1) & (c[1::2] <= 5)).all()
    assert float(est[EST[2]].min()) >= 0.1 and float(est[EST[2]].max()) < 1.0
    for s in range(3):
        y = synth.synth_isda_targets(4, s)
        assert int((y[:, 10 + s] != 0).sum()) == 3 and y[1, 7] == 1.0 and not y[3].any()
