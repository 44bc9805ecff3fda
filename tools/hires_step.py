"""One VLMo-Base forward_features fwd + bwd step at higher resolution: 384 px (B 32) and 480 px (B 16), timed the way
bench.py times its backbone objective (warm-up steps, then a wall-clock window over K steps closed by a device
synchronisation; the loss is (x * R).sum() with a fixed random R).

    python tools/hires_step.py [--steps 10] [--warmup 3] [--res 384:32,480:16] [--json out.json]"""
import argparse
import json
import os
import sys
import time
from functools import partial

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from exploremultimodal_amd import synth  # noqa: E402
from exploremultimodal_amd.vlmo import VLMO, LayerNorm  # noqa: E402


def run(res, B, steps, warmup):
    mc = synth.make_config('base', img_size=res).model
    model = VLMO(img_size=mc.img_size, patch_size=mc.patch_size, embed_dim=mc.embed_dim, depth=mc.depth,
                 num_heads=mc.num_heads, mlp_ratio=mc.mlp_ratio, qkv_bias=True, drop_rate=0.1, attn_drop_rate=0.1,
                 drop_path_rate=0.1, norm_layer=partial(LayerNorm, eps=1e-12), init_values=mc.init_values,
                 vocab_size=mc.vocab_size, max_text_len=mc.max_text_len, fusion_layer=mc.fusion_layer)
    model.load_state_dict(synth.synth_backbone_state_dict(mc, 0, [('v', 'l', 'vl')] * mc.depth))
    model = model.cuda().train()
    batch = synth.synth_batch(mc, B, seed=1234, mim=False)
    P = synth.num_img_tokens(mc)
    img, ids, tmask = batch['image'].cuda(), batch['text_ids'].cuda(), batch['text_mask'].cuda()
    imask = torch.ones(B, P, dtype=torch.int64, device='cuda')
    R = torch.randn(B, mc.max_text_len + P, mc.embed_dim, device='cuda') / (B * 1000.0)

    def step():
        for p in model.parameters():
            p.grad = None
        x, _ = model.forward_features(img=img, txt=ids, img_attn_masks=imask, txt_attn_masks=tmask)
        loss = (x * R).sum()
        loss.backward()
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
    return dict(img_size=res, B=B, image_tokens=P, fused_tokens=P + mc.max_text_len, ms_per_step=round(dt * 1e3, 2),
                pairs_per_s=round(B / dt, 1), peak_mem_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--res', default='384:32,480:16')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    rows = []
    for item in args.res.split(','):
        res, B = (int(v) for v in item.split(':'))
        torch.cuda.reset_peak_memory_stats()
        r = run(res, B, args.steps, args.warmup)
        rows.append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
