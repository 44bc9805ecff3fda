"""attnmap.attention_gradcam (HIP, vlmo_attn_gradcam) against the torch form of Grad-CAM on the attention maps, on one GPU.

The torch form is what a hook and retain_grad() on `attn` cost in the reference: P = softmax(q k^T * scale + mask)
materialised in fp32, P.requires_grad_(), ctx = P @ v, autograd.grad((ctx * dctx).sum(), P), then P * relu(grad).
Two cases, as tools/attnmap_bench.py: VLMo-Base fused layers (64 sequences x 12 heads x 261 tokens: K and V resident)
and 480 px (16 x 12 x 965: K resident, V streamed).  Whole calls between device events (the HIP form includes its output
allocation, the torch form its fp32 casts), all forms back to back in every round; median, minimum and maximum over the
rounds.  The kernel is bound by its output, as vlmo_attn_probs is, so that kernel's time on the same shapes is printed
beside it: it is the number to hold the new one against.  Prints a markdown table and one JSON line.

    python tools/gradcam_bench.py [--rounds 9] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from exploremultimodal_amd import attnmap

DEV = 'cuda'
CASES = [('Base, fused', 64, 12, 261), ('480 px', 16, 12, 965)]


def torch_gradcam(qkv, dctx, nseq, heads, n, bias, scale):
    x = qkv.view(nseq, n, 3, heads, 64).float()
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    P = torch.softmax(q @ k.transpose(-1, -2) * scale + bias, -1).requires_grad_()
    ctx = P @ v
    G, = torch.autograd.grad((ctx * dctx.view(nseq, n, heads, 64).transpose(1, 2).float()).sum(), P)
    return P.detach() * G.clamp_min(0) * (bias == 0)


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    del out
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    rows = []
    for name, nseq, heads, n in CASES:
        qkv = torch.randn(nseq * n, 3 * 64 * heads, device=DEV, generator=gen).bfloat16()
        dctx = torch.randn(nseq * n, 64 * heads, device=DEV, generator=gen).bfloat16()
        seg = torch.tensor([[s * n, n, 0, 0] for s in range(nseq)], dtype=torch.int32, device=DEV)
        km = torch.ones(nseq * n, dtype=torch.int32, device=DEV)
        km.view(nseq, n)[1::2, n - 9:] = 0                       # every other sequence has a padded tail
        bias = torch.zeros(nseq, 1, 1, n, device=DEV).masked_fill(km.view(nseq, 1, 1, n) == 0, float('-inf'))
        scale = 0.125
        forms = {'cam': lambda: attnmap.attention_gradcam(qkv, dctx, seg, nseq, n, heads, keymask=km),
                 'grad': lambda: attnmap.attention_gradcam(qkv, dctx, seg, nseq, n, heads, keymask=km, kind='grad'),
                 'cam_head_mean': lambda: attnmap.attention_gradcam(qkv, dctx, seg, nseq, n, heads, keymask=km,
                                                                    head_mean=True),
                 'probs': lambda: attnmap.attention_probs(qkv, seg, nseq, n, heads, keymask=km),
                 'torch': lambda: torch_gradcam(qkv, dctx, nseq, heads, n, bias, scale)}
        ref = forms['torch']()
        diff = (forms['cam']() - ref).abs().max().item() / ref.abs().max().item()      # also the warm-up
        del ref
        for k in ('grad', 'cam_head_mean', 'probs'):
            forms[k]()
        times = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                times[k].append(timed(fn))
        out_bytes = 4 * nseq * heads * n * n
        row = dict(case=name, sequences=nseq, heads=heads, tokens=n, out_mb=out_bytes / 1e6, rounds=args.rounds,
                   max_diff_vs_torch_rel_to_max=diff)
        for k, v in times.items():
            row[k + '_ms'], row[k + '_min_ms'], row[k + '_max_ms'] = statistics.median(v), min(v), max(v)
        row['cam_gbs'] = out_bytes / row['cam_ms'] / 1e6
        rows.append(row)
        del qkv, dctx, bias
        torch.cuda.empty_cache()
    f3 = lambda r, k: f"{r[k + '_ms']:.3f} ({r[k + '_min_ms']:.3f} - {r[k + '_max_ms']:.3f})"
    print('| case | seq x heads x tokens | output MB | cam ms (min - max) | output GB/s | grad ms | cam head_mean ms | '
          'attention_probs ms | torch autograd ms |')
    print('|---|---|---|---|---|---|---|---|---|')
    for r in rows:
        print(f"| {r['case']} | {r['sequences']} x {r['heads']} x {r['tokens']} | {r['out_mb']:.0f} | {f3(r, 'cam')} | "
              f"{r['cam_gbs']:.0f} | {f3(r, 'grad')} | {f3(r, 'cam_head_mean')} | {f3(r, 'probs')} | {f3(r, 'torch')} |")
    line = json.dumps({'gradcam_bench': rows})
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
