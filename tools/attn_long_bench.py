"""Streaming attention kernels at VLMo-Base heads (12, d 768): forward and backward at N in {577, 617, 941, 1024}
(384 px image / fused, 480 px fused, the cap), and the resident kernels at 261 (224 px fused) for reference.

    python tools/attn_long_bench.py [--batch B] [--drop 0.1] [--json out.json]

One launch covers B sequences of N tokens.  TFLOP/s counts 4 N^2 64 flops per (sequence, head) for the forward and
10 N^2 64 for the backward (its five products), padding not included."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from exploremultimodal_amd import hip  # noqa: E402

H, D = 12, 768


def timeit(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def run(B, N, drop, reps):
    M = B * N
    g = torch.Generator(device='cuda').manual_seed(N)
    qkv = torch.randn(M, 3 * D, device='cuda', generator=g).bfloat16()
    seg = torch.tensor([[b * N, N, 0, 0] for b in range(B)], dtype=torch.int32, device='cuda')
    km = torch.ones(M, dtype=torch.int32, device='cuda')
    ctx = torch.empty(M, D, device='cuda', dtype=torch.bfloat16)
    lse = torch.empty(B * H, ((N + 31) // 32) * 32, device='cuda')
    dctx = torch.randn(M, D, device='cuda', generator=g).bfloat16()
    dqkv = torch.empty(M, 3 * D, device='cuda', dtype=torch.bfloat16)
    dp = hip.drop_params(drop, True)
    tf = timeit(lambda: hip.attn_fwd(qkv, seg, B, km, ctx, lse, H, D, N, 0.125, drop=dp, seed=1), reps)
    tb = timeit(lambda: hip.attn_bwd(qkv, ctx, dctx, lse, seg, B, km, dqkv, H, D, N, 0.125, drop=dp, seed=1), reps)
    fl = B * H * N * N * 64
    kern = lambda lim: 'streaming' if N > lim else 'resident'
    return dict(N=N, B=B, drop=drop, fwd_us=round(tf * 1e6, 1), fwd_tflops=round(4 * fl / tf / 1e12, 1),
                bwd_us=round(tb * 1e6, 1), bwd_tflops=round(10 * fl / tb / 1e12, 1),
                fwd_kernel=kern(512), bwd_kernel=kern(288))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--drop', type=float, default=0.1)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    rows = []
    for N in (261, 577, 617, 941, 1024):
        r = run(args.batch, N, args.drop, args.reps)
        rows.append(r)
        print(f"N={N:5d} B={args.batch} drop={args.drop}: fwd {r['fwd_us']:8.1f} us {r['fwd_tflops']:6.1f} TF/s "
              f"({r['fwd_kernel']}) | bwd {r['bwd_us']:8.1f} us {r['bwd_tflops']:6.1f} TF/s ({r['bwd_kernel']})", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
