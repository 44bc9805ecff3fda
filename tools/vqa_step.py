"""VQAv2 fine-tuning on the GPU: (1) one full VLMo-Base fine-tune step -- VlmoModule.forward with loss_names ['vqa'],
backward and FusedAdam with the three learning-rate groups of conf/train/finetune_vqa.yaml (base_lr 3e-6,
lr_mult_head 50, lr_mult_fusion 5) and clip 5.0 through NativeScalerWithGradNormCount -- at 384 px (B 32) and 480 px
(B 16), timed like tools/hires_step.py; (2) an interleaved A/B of the classifier + loss alone: heads.VQAHeadFn (HIP)
against a torch restatement of the reference head (nn.Sequential + BCE-with-logits + compute_vqa_score), forward +
backward, at B in {16, 64, 512} with the Base (768) and Large (1024) widths.

    python tools/vqa_step.py [--steps 10] [--warmup 3] [--res 384:32,480:16] [--ab-iters 50] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from exploremultimodal_amd import objectives, optim, synth  # noqa: E402
from exploremultimodal_amd.build import build_model  # noqa: E402

VS = 3129


def run_step(res, B, steps, warmup):
    cfg = synth.make_config('base', loss_names=['vqa'], phase='finetune_vqa', img_size=res, drop_rate=0.1,
                            attn_drop_rate=0.1, drop_path_rate=0.1)
    mc = cfg.model
    model = build_model(cfg)
    sd = {'transformer.' + k: v for k, v in synth.synth_backbone_state_dict(mc, 0).items()}
    sd.update(synth.synth_head_state_dict(mc, 0, ['vqa']))
    model.load_state_dict(sd, strict=False)
    model = model.cuda().train()
    host = synth.synth_batch(mc, B, seed=1234, mim=False)
    host['vqa_targets'] = synth.synth_vqa_targets(B, VS)
    objectives.attach_row_indices(host)
    batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in host.items()}
    groups = optim.get_parameter_groups(model, base_lr=3e-6, lr_mult_head=50, lr_mult_fusion=5, weight_decay=0.01,
                                        skip_list=model.no_weight_decay())
    opt = optim.FusedAdam(groups, betas=(0.9, 0.98), eps=1e-8)
    scaler = optim.NativeScalerWithGradNormCount()
    params = [p for p in model.parameters() if p.requires_grad]

    def step():
        opt.zero_grad(set_to_none=True)
        loss = model(dict(batch))['vqa_task_loss']
        scaler(loss, opt, clip_grad=5.0, parameters=params, update_grad=True)
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    assert torch.isfinite(loss).item(), 'non-finite loss'
    P = synth.num_img_tokens(mc)
    return dict(kind='finetune_step', img_size=res, B=B, fused_tokens=P + mc.max_text_len, lr_groups=len(groups),
                ms_per_step=round(dt * 1e3, 2), pairs_per_s=round(B / dt, 1),
                peak_mem_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))


def _head(hs):
    torch.manual_seed(hs)
    head = torch.nn.Sequential(torch.nn.Linear(hs, 2 * hs), torch.nn.LayerNorm(2 * hs, eps=1e-12), torch.nn.GELU(),
                               torch.nn.Linear(2 * hs, VS)).cuda()
    return head


def run_ab(hs, B, iters, rounds=5):
    from exploremultimodal_amd.derived import Holder
    from exploremultimodal_amd.heads import VQAHeadFn
    head = _head(hs)
    sh = Holder()
    x = torch.randn(B, hs, device='cuda', requires_grad=True)
    y = synth.synth_vqa_targets(B, VS).cuda()
    fc1, ln, _, fc2 = head

    def hip_step():
        logits, loss, _, score = VQAHeadFn.apply(x, fc1.weight, fc1.bias, ln.weight, ln.bias, fc2.weight, fc2.bias, y,
                                                 ln.eps, torch.float32, sh)
        loss.backward()
        return score.sum() / B

    def torch_step():
        logits = head(x)
        loss = F.binary_cross_entropy_with_logits(logits, y) * VS
        score, _ = objectives.compute_vqa_score(logits, y)
        loss.backward()
        return score

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e6

    for fn in (hip_step, torch_step):
        for _ in range(5):
            fn()
    hip_us, torch_us = [], []
    for _ in range(rounds):             # interleaved: both sides see the same clock / thermal state
        hip_us.append(timed(hip_step))
        torch_us.append(timed(torch_step))
    h, t = statistics.median(hip_us), statistics.median(torch_us)
    return dict(kind='head_ab', hidden=hs, B=B, hip_us=round(h, 1), torch_us=round(t, 1), speedup=round(t / h, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--res', default='384:32,480:16')
    ap.add_argument('--ab-iters', type=int, default=50)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    rows = []
    for hs in (768, 1024):
        for B in (16, 64, 512):
            r = run_ab(hs, B, args.ab_iters)
            rows.append(r)
            print(json.dumps(r), flush=True)
    for item in filter(None, args.res.split(',')):
        res, B = (int(v) for v in item.split(':'))
        torch.cuda.reset_peak_memory_stats()
        r = run_step(res, B, args.steps, args.warmup)
        rows.append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
