"""Reference fixture of VQAv2 fine-tuning with ISDA (tests/test_isda_cpu.py, tests/test_isda_module_gpu.py).

    python tools/gen_isda_golden.py            # writes tests/golden/vqa_isda_mini.npz

Runs the unmodified reference VlmoModule (models/vlmo/vlmo_module.py) with loss_names = ['vqa'], phase =
'finetune_vqa', isda_lambda 7.5, epochs 2, cur_epoch 1 (ratio 3.75) on the machine that holds the reference, through
the committed generator helpers (oracle.gen_golden: the reference path, the timm stand-in, grad_probe).  Weights: the
key-addressed synthetic backbone and ISDA head (synth_isda_head_state_dict) and the seeded estimator state
(synth_isda_estimator).  Three consecutive training steps (dropout 0) with the same weights, each on its own batch
(synth_batch seed 1234 + s) and targets (synth_isda_targets(B, s)); the estimator carries over.  Per step s:

  s<s>.vqa_targets, s<s>.cls_feats                        the targets and the pooled features fed to the head
  s<s>.ret.vqa_{logits,task_loss,mean_score,count}        the reference's outputs (augmented logits)
  s<s>.z                                                  the pre-ISDA logits (a hook on vqa_last)
  s<s>.k                                                  the arg-max class of each target row
  s<s>.count, s<s>.touched, s<s>.mean_rows, s<s>.cov_rows  estimator after the step: count [vs], the classes with a
                                                          member row this step and their mean / cov rows
  s<s>.grad_norm.<p>, s<s>.grad_probe.<p>                 every parameter with a gradient
  s<s>.grad_rows_idx, s<s>.grad_rows                      full rows of vqa_last.weight's gradient for touched and k
  eval.vqa_logits, eval.vqa_task_loss, eval.keys          eval mode on step 0's batch (no augmentation, no update)
  keys                                                    the reference module's state-dict keys

The mini preset at 224 px, batch 4."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden  # noqa: E402

B, STEPS = 4, 3
TRAIN = dict(isda_lambda=7.5, epochs=2, cur_epoch=1)


def run(seed=0):
    from oracle import synth
    from models.build import build_model
    cfg = synth.make_config('mini', loss_names=['vqa'], phase='finetune_vqa', img_size=224)
    for k, v in TRAIN.items():
        setattr(cfg.train, k, v)
    mc = cfg.model
    mc.mlp_ratio = int(mc.mlp_ratio)
    model = build_model(cfg)
    vs, A = cfg.data.vqav2_label_size, 2 * mc.embed_dim
    sd = {'transformer.' + k: v for k, v in synth.synth_backbone_state_dict(mc, seed).items()}
    sd.update(synth.synth_isda_head_state_dict(mc, seed))
    sd.update(synth.synth_isda_estimator(A, vs, seed))
    r = model.load_state_dict(sd, strict=False)
    assert not r.unexpected_keys and not r.missing_keys, (r.unexpected_keys, r.missing_keys)
    rec = {'keys': np.array(list(model.state_dict().keys()))}
    seen = {}
    model.vqa_classifier.register_forward_hook(lambda m, i, o: seen.__setitem__('feats', i[0].detach().clone()))
    model.vqa_last.register_forward_hook(lambda m, i, o: seen.__setitem__('z', o.detach().clone()))
    est = model.isda_head.estimator
    model.train()
    for s in range(STEPS):
        batch = synth.synth_batch(mc, B, seed=1234 + s, mim=False)
        y = synth.synth_isda_targets(B, s, vs)
        batch['vqa_targets'] = y
        model.zero_grad(set_to_none=True)
        ret = model(dict(batch))
        assert set(ret) == {'vqa_logits', 'vqa_count', 'vqa_task_loss', 'vqa_targets', 'vqa_mean_score'}, sorted(ret)
        p = f's{s}.'
        rec[p + 'vqa_targets'] = y.numpy().astype(np.float32)
        rec[p + 'cls_feats'] = seen['feats'].numpy().astype(np.float32)
        rec[p + 'z'] = seen['z'].numpy().astype(np.float32)
        rec[p + 'ret.vqa_logits'] = ret['vqa_logits'].detach().numpy().astype(np.float32)
        rec[p + 'ret.vqa_task_loss'] = np.float64(ret['vqa_task_loss'].item())
        rec[p + 'ret.vqa_mean_score'] = np.float64(ret['vqa_mean_score'].item())
        rec[p + 'ret.vqa_count'] = np.int64(ret['vqa_count'])
        k = torch.max(y, 1)[1]
        touched = (y != 0).any(0).nonzero().flatten()
        rec[p + 'k'] = k.numpy().astype(np.int64)
        rec[p + 'touched'] = touched.numpy().astype(np.int64)
        rec[p + 'count'] = est.count.numpy().astype(np.float32)
        rec[p + 'mean_rows'] = est.mean[touched].numpy().astype(np.float32)
        rec[p + 'cov_rows'] = est.cov[touched].numpy().astype(np.float32)
        ret['vqa_task_loss'].backward()
        for name, prm in model.named_parameters():
            if prm.grad is None:
                continue
            g = prm.grad.detach()
            rec[p + 'grad_norm.' + name] = np.float64(g.double().norm().item())
            rec[p + 'grad_probe.' + name] = np.float64((g.double() * gen_golden.grad_probe(name, g.shape).double()).sum().item())
        rows = torch.unique(torch.cat([touched, k]))
        rec[p + 'grad_rows_idx'] = rows.numpy().astype(np.int64)
        rec[p + 'grad_rows'] = model.vqa_last.weight.grad[rows].numpy().astype(np.float32)
    before = {k: v.clone() for k, v in est.state_dict().items()}
    model.eval()
    batch = synth.synth_batch(mc, B, seed=1234, mim=False)
    batch['vqa_targets'] = torch.from_numpy(rec['s0.vqa_targets'])
    with torch.no_grad():
        ev = model(dict(batch))
    assert all(torch.equal(before[k], v) for k, v in est.state_dict().items())
    rec['eval.vqa_logits'] = ev['vqa_logits'].numpy().astype(np.float32)
    rec['eval.vqa_task_loss'] = np.float64(ev['vqa_task_loss'].item())
    rec['eval.keys'] = np.array(sorted(ev))
    rec['meta.B'] = np.int64(B)
    rec['meta.ratio'] = np.float64(TRAIN['isda_lambda'] * TRAIN['cur_epoch'] / TRAIN['epochs'])
    out = os.path.join(gen_golden.OUT, 'vqa_isda_mini.npz')
    np.savez_compressed(out, **rec)
    aug = np.abs(rec['s0.ret.vqa_logits'] - rec['s0.z']).max()
    print(f'wrote vqa_isda_mini.npz with {len(rec)} arrays, {os.path.getsize(out)} bytes; max |aug| step 0 {aug:.4g}; '
          f'losses {[round(float(rec[f"s{s}.ret.vqa_task_loss"]), 5) for s in range(STEPS)]}')


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    sys.path.insert(0, gen_golden.REF)
    gen_golden._install_timm_standin()
    run()


if __name__ == '__main__':
    main()
