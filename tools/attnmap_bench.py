"""attnmap.attention_probs (HIP, vlmo_attn_probs) against torch.softmax(q @ k^T * scale + mask, -1) in fp32 on one GPU.

Two cases: VLMo-Base fused layers (64 sequences x 12 heads x 261 tokens: 209 MB of probabilities) and 480 px (16 x 12 x
965: 715 MB).  Whole calls between device events (the HIP form includes its output allocation, the torch form its
fp32 casts of q and k), both forms back to back in every round, the median over the rounds.  The kernel is bound by its
output, so the table gives output GB/s next to the milliseconds; the yardstick is the plain-write ceiling of DESIGN
section 5 (6.3 - 6.9 TB/s).  Also times head_mean=True (1 / heads of the output).  Prints a markdown table and one JSON line.

    python tools/attnmap_bench.py [--rounds 9] [--out FILE.json]
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


def torch_probs(qkv, nseq, heads, n, bias, scale):
    x = qkv.view(nseq, n, 3, heads, 64).float()
    q, k = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2)
    return torch.softmax(q @ k.transpose(-1, -2) * scale + bias, -1)


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
        seg = torch.tensor([[s * n, n, 0, 0] for s in range(nseq)], dtype=torch.int32, device=DEV)
        km = torch.ones(nseq * n, dtype=torch.int32, device=DEV)
        km.view(nseq, n)[1::2, n - 9:] = 0                       # every other sequence has a padded tail
        bias = torch.zeros(nseq, 1, 1, n, device=DEV).masked_fill(km.view(nseq, 1, 1, n) == 0, float('-inf'))
        scale = 0.125
        forms = {'hip': lambda: attnmap.attention_probs(qkv, seg, nseq, n, heads, keymask=km),
                 'hip_head_mean': lambda: attnmap.attention_probs(qkv, seg, nseq, n, heads, keymask=km, head_mean=True),
                 'torch': lambda: torch_probs(qkv, nseq, heads, n, bias, scale)}
        diff = (forms['hip']() - forms['torch']()).abs().max().item()        # also the warm-up
        forms['hip_head_mean']()
        times = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                times[k].append(timed(fn))
        out_bytes = 4 * nseq * heads * n * n
        row = dict(case=name, sequences=nseq, heads=heads, tokens=n, out_mb=out_bytes / 1e6, rounds=args.rounds,
                   max_abs_diff_vs_torch=diff)
        for k, v in times.items():
            row[k + '_ms'], row[k + '_min_ms'] = statistics.median(v), min(v)
        row['hip_gbs'] = out_bytes / row['hip_ms'] / 1e6
        row['torch_gbs'] = out_bytes / row['torch_ms'] / 1e6
        rows.append(row)
        del qkv, bias
        torch.cuda.empty_cache()
    print('| case | seq x heads x tokens | output MB | attention_probs ms | output GB/s | head_mean ms | torch fp32 ms | torch GB/s |')
    print('|---|---|---|---|---|---|---|---|')
    for r in rows:
        print(f"| {r['case']} | {r['sequences']} x {r['heads']} x {r['tokens']} | {r['out_mb']:.0f} | {r['hip_ms']:.3f} | "
              f"{r['hip_gbs']:.0f} | {r['hip_head_mean_ms']:.3f} | {r['torch_ms']:.3f} | {r['torch_gbs']:.0f} |")
    line = json.dumps({'attnmap_bench': rows})
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
