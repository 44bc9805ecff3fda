"""retrieval.sim_topk (HIP, fused) against the torch form (q @ g.t() * scale).topk(k) on one GPU: time and peak memory.

Shapes: the two directions of the COCO 5k test split (25 000 captions x 5 000 images, D 256, K 10) and one large gallery
(100 000 x 100 000 by default), where torch runs chunked over the queries so that its score slab stays near 1 GB.
Each round times both forms back to back (interleaved), the table shows the median over the rounds; peak memory is
torch.cuda.max_memory_allocated above the inputs.  Prints a markdown table and one JSON line.

    python tools/retrieval_bench.py [--rounds 7] [--big 100000] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from exploremultimodal_amd import retrieval as R

DEV = 'cuda'


def torch_topk(q, g, k, scale, chunk):
    if chunk >= q.shape[0]:
        return (q @ g.t() * scale).topk(k)
    vals, idxs = [], []
    for r0 in range(0, q.shape[0], chunk):
        v, i = (q[r0:r0 + chunk] @ g.t() * scale).topk(k)
        vals.append(v)
        idxs.append(i)
    return torch.cat(vals), torch.cat(idxs)


def timed(fn):
    """-> (milliseconds, peak bytes above what was allocated before the call)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return a.elapsed_time(b), peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--big', type=int, default=100000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    shapes = [('coco5k t2i', 25000, 5000, args.rounds), ('coco5k i2t', 5000, 25000, args.rounds)]
    if args.big > 0:
        shapes.append((f'{args.big // 1000}k x {args.big // 1000}k', args.big, args.big, min(args.rounds, 3)))
    D, K, scale = 256, 10, 1.0
    rows = []
    for name, Nq, Ng, rounds in shapes:
        q = torch.nn.functional.normalize(torch.randn(Nq, D, device=DEV, generator=gen), dim=1)
        g = torch.nn.functional.normalize(torch.randn(Ng, D, device=DEV, generator=gen), dim=1)
        chunk = max(1, min(Nq, (1 << 28) // Ng))             # torch's score slab: at most 2^28 floats (1 GB)
        hip_fn = lambda: R.sim_topk(q, g, K, scale)
        torch_fn = lambda: torch_topk(q, g, K, scale, chunk)
        hip_fn(), torch_fn()                                 # warm-up: allocator, kernel load
        th, tt, mh, mt = [], [], 0, 0
        for _ in range(rounds):
            ms, pk = timed(hip_fn)
            th.append(ms)
            mh = max(mh, pk)
            ms, pk = timed(torch_fn)
            tt.append(ms)
            mt = max(mt, pk)
        _, ih = hip_fn()
        _, it = torch_fn()
        agree = (ih == it).all(1).float().mean().item()      # torch breaks ties and rounds its scores its own way
        rows.append(dict(shape=name, Nq=Nq, Ng=Ng, D=D, K=K, hip_ms=statistics.median(th), torch_ms=statistics.median(tt),
                         hip_min_ms=min(th), torch_min_ms=min(tt), hip_peak_mb=mh / 1e6, torch_peak_mb=mt / 1e6,
                         torch_chunk=chunk, rounds=rounds, rows_equal=agree))
        del q, g
        torch.cuda.empty_cache()
    print('| shape | Nq x Ng | sim_topk ms | torch ms | sim_topk peak MB | torch peak MB | rows with equal indices |')
    print('|---|---|---|---|---|---|---|')
    for r in rows:
        print(f"| {r['shape']} | {r['Nq']} x {r['Ng']} | {r['hip_ms']:.2f} | {r['torch_ms']:.2f} | {r['hip_peak_mb']:.1f} | "
              f"{r['torch_peak_mb']:.1f} | {r['rows_equal']:.4f} |")
    line = json.dumps({'retrieval_bench': rows})
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
