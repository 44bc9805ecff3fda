"""Reference fixtures of VQAv2 fine-tuning (tests/test_vqa_module_gpu.py).

    python tools/gen_vqa_golden.py            # writes tests/golden/vqa_mini{,_480}.npz

Runs the unmodified reference VlmoModule (models/vlmo/vlmo_module.py) with loss_names = ['vqa'] and
phase = 'finetune_vqa' on the machine that holds the reference, through the committed generator helpers
(oracle.gen_golden: the reference path, the timm stand-in, grad_probe), on the key-addressed synthetic weights of
exploremultimodal_amd.synth: backbone, pooler and the VQA classifier (3129 answers).  Per case, in training mode with
dropout 0:

  vqa_targets [B, 3129]                                                 synth_vqa_targets, plus an answer (1.0) at the
                                                                        reference's arg-max on even rows but the last
                                                                        (so the score is not zero everywhere)
  ret.vqa_logits, ret.vqa_task_loss, ret.vqa_mean_score, ret.vqa_count   the reference's outputs
  logits_top2_gap [B]                                                   top-2 logit gap per row (near-tie arg-max)
  grad_norm.<p>, grad_probe.<p>                                         every parameter with a gradient
  grad.<p>                                                              full gradients of parameters <= 4 096 elements
  eval.vqa_logits, eval.keys                                            eval mode, all targets zero

vqa_mini: the mini preset at 224 px, batch 4 (213 fused tokens); vqa_mini_480: 480 px, batch 2, 40 text tokens
(941 fused tokens)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden  # noqa: E402

FULL_GRAD_MAX = 4096
CASES = {
    'vqa_mini': dict(preset='mini', B=4, img_size=224),
    'vqa_mini_480': dict(preset='mini', B=2, img_size=480, max_text_len=40),
}


def run_case(name, preset, B, seed=0, **model_over):
    from oracle import synth
    from models.build import build_model
    cfg = synth.make_config(preset, loss_names=['vqa'], phase='finetune_vqa', **model_over)
    mc = cfg.model
    mc.mlp_ratio = int(mc.mlp_ratio)
    model = build_model(cfg)
    sd = {'transformer.' + k: v for k, v in synth.synth_backbone_state_dict(mc, seed).items()}
    sd.update(synth.synth_head_state_dict(mc, seed, ['vqa']))
    r = model.load_state_dict(sd, strict=False)
    assert not r.unexpected_keys and not r.missing_keys, (r.unexpected_keys, r.missing_keys)
    batch = synth.synth_batch(mc, B, seed=1234, mim=False)
    batch['vqa_targets'] = synth.synth_vqa_targets(B, cfg.data.vqav2_label_size)
    with torch.no_grad():
        am = model.eval()(dict(batch))['vqa_logits'].argmax(1)
    for b in range(0, B - 1, 2):
        batch['vqa_targets'][b, am[b]] = 1.0
    rec = {'vqa_targets': batch['vqa_targets'].numpy().astype(np.float32)}
    model.train()
    ret = model(dict(batch))
    assert set(ret) == {'vqa_logits', 'vqa_count', 'vqa_task_loss', 'vqa_targets', 'vqa_mean_score'}, sorted(ret)
    lg = ret['vqa_logits'].detach()
    rec['ret.vqa_logits'] = lg.numpy().astype(np.float32)
    rec['ret.vqa_task_loss'] = np.float64(ret['vqa_task_loss'].item())
    rec['ret.vqa_mean_score'] = np.float64(ret['vqa_mean_score'].item())
    rec['ret.vqa_count'] = np.int64(ret['vqa_count'])
    t2 = lg.topk(2, dim=1).values
    rec['logits_top2_gap'] = (t2[:, 0] - t2[:, 1]).numpy().astype(np.float32)
    model.zero_grad(set_to_none=True)
    ret['vqa_task_loss'].backward()
    for k, p in model.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.detach()
        rec['grad_norm.' + k] = np.float64(g.double().norm().item())
        rec['grad_probe.' + k] = np.float64((g.double() * gen_golden.grad_probe(k, g.shape).double()).sum().item())
        if g.numel() <= FULL_GRAD_MAX:
            rec['grad.' + k] = g.numpy().astype(np.float32)
    # eval mode, no answer in the batch: the reference returns the logits and the count only
    model.eval()
    with torch.no_grad():
        ev = model(dict(batch, vqa_targets=torch.zeros_like(batch['vqa_targets'])))
    rec['eval.vqa_logits'] = ev['vqa_logits'].numpy().astype(np.float32)
    rec['eval.keys'] = np.array(sorted(ev))
    rec['meta.B'] = np.int64(B)
    np.savez_compressed(os.path.join(gen_golden.OUT, f'{name}.npz'), **rec)
    print(f'wrote {name}.npz with {len(rec)} arrays; loss {rec["ret.vqa_task_loss"]:.6f} '
          f'score {rec["ret.vqa_mean_score"]:.4f}')


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    sys.path.insert(0, gen_golden.REF)
    gen_golden._install_timm_standin()
    for name, kw in CASES.items():
        kw = dict(kw)
        run_case(name, kw.pop('preset'), kw.pop('B'), **kw)


if __name__ == '__main__':
    main()
