"""VLMO.attention_relevance (rows carried through vlmo_relevance_step inside the pass) against the by-hand form on one GPU:
attention_gradcam (or attention_maps) for ALL layers with head_mean=True, which keeps L maps, then a torch.baddbmm chain
over them from the top layer down -- per-modality layers as two products on column slices.

VLMo-Base at 64 pairs (224 px, 261 fused tokens) and at 480 px (16 pairs, 965 fused tokens), methods 'gradcam' (the ITM-like
score is a fixed random projection of the text CLS) and 'rollout', queries (0, 1) -- the text [CLS] -- and None (all rows).
Whole calls between device events, the new and the by-hand form back to back in every round, in the same process on the
same card; median (min - max) of the rounds after the warm-up rounds.  Both forms run the same forward (and backward): the
difference is the propagation and the memory the maps take.  Prints a markdown table and one JSON line.

    python tools/relevance_bench.py [--rounds 9] [--warmup 3] [--cases 224:64,480:16] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
from functools import partial

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from exploremultimodal_amd import attnmap, synth  # noqa: E402
from exploremultimodal_amd.vlmo import VLMO, LayerNorm  # noqa: E402

DEV = 'cuda'


def build(res):
    mc = synth.make_config('base', img_size=res).model
    model = VLMO(img_size=mc.img_size, patch_size=mc.patch_size, embed_dim=mc.embed_dim, depth=mc.depth,
                 num_heads=mc.num_heads, mlp_ratio=mc.mlp_ratio, qkv_bias=True, norm_layer=partial(LayerNorm, eps=1e-12),
                 init_values=mc.init_values, vocab_size=mc.vocab_size, max_text_len=mc.max_text_len,
                 fusion_layer=mc.fusion_layer)
    model.load_state_dict(synth.synth_backbone_state_dict(mc, 0, [('v', 'l', 'vl')] * mc.depth))
    return model.to(DEV).eval(), mc


def by_hand(model, score, kw, T, N, queries, method):
    """What a user of attention_gradcam / attention_maps writes today."""
    alpha, beta = attnmap.METHODS[method]
    if method == 'gradcam':
        maps = model.attention_gradcam(score, kind='cam', head_mean=True, **kw)
    else:
        maps = model.attention_maps(head_mean=True, **kw)
    q0, nq = (0, N) if queries is None else queries
    B = kw['txt'].shape[0]
    X = torch.eye(N, device=DEV)[q0:q0 + nq].expand(B, nq, N).contiguous()
    for i in sorted(maps, reverse=True):
        m = maps[i]
        if isinstance(m, dict):
            X = torch.cat([torch.baddbmm(X[:, :, :T], X[:, :, :T], m['txt'][:, 0], beta=alpha, alpha=beta),
                           torch.baddbmm(X[:, :, T:], X[:, :, T:], m['img'][:, 0], beta=alpha, alpha=beta)], dim=2)
        else:
            X = torch.baddbmm(X, X, m[:, 0], beta=alpha, alpha=beta)
    return X


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
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--cases', default='224:64,480:16')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rows = []
    for item in args.cases.split(','):
        res, B = (int(v) for v in item.split(':'))
        model, mc = build(res)
        batch = synth.synth_batch(mc, B, seed=1234, mim=False)
        T, P = mc.max_text_len, synth.num_img_tokens(mc)
        N = T + P
        kw = dict(img=batch['image'].to(DEV), txt=batch['text_ids'].to(DEV), txt_attn_masks=batch['text_mask'].to(DEV),
                  img_attn_masks=torch.ones(B, P, dtype=torch.int64, device=DEV))
        w = torch.randn(mc.embed_dim, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
        score = lambda x, mask=None: (x[:, 0] @ w).sum()        # noqa: E731
        for method in ('gradcam', 'rollout'):
            for queries in ((0, 1), None):
                forms = {'relevance': lambda: model.attention_relevance(score, queries=queries, method=method, **kw),
                         'by_hand': lambda: by_hand(model, score, kw, T, N, queries, method)}
                torch.cuda.reset_peak_memory_stats()
                ref = forms['by_hand']()
                hand_gib = torch.cuda.max_memory_allocated() / 2 ** 30
                torch.cuda.reset_peak_memory_stats()
                got = forms['relevance']()
                new_gib = torch.cuda.max_memory_allocated() / 2 ** 30
                diff = ((got - ref).abs().max() / ref.abs().max()).item()
                del got, ref
                times = {k: [] for k in forms}
                for r in range(args.warmup + args.rounds):
                    for k, fn in forms.items():
                        t = timed(fn)
                        if r >= args.warmup:
                            times[k].append(t)
                row = dict(img_size=res, pairs=B, tokens=N, layers=mc.depth, method=method,
                           queries='all' if queries is None else list(queries), rounds=args.rounds, warmup=args.warmup,
                           max_diff_rel_to_max=diff, relevance_peak_gib=round(new_gib, 2), by_hand_peak_gib=round(hand_gib, 2))
                for k, v in times.items():
                    row[k + '_ms'], row[k + '_min_ms'], row[k + '_max_ms'] = statistics.median(v), min(v), max(v)
                rows.append(row)
                print(json.dumps(row), flush=True)
        del model, kw
        torch.cuda.empty_cache()
    f3 = lambda r, k: f"{r[k + '_ms']:.1f} ({r[k + '_min_ms']:.1f} - {r[k + '_max_ms']:.1f})"      # noqa: E731
    print('| px, pairs x tokens | method | queries | attention_relevance ms (min - max) | by hand ms (min - max) | '
          'peak GiB new / by hand | max diff / max |')
    print('|---|---|---|---|---|---|---|')
    for r in rows:
        print(f"| {r['img_size']}, {r['pairs']} x {r['tokens']} | {r['method']} | {r['queries']} | {f3(r, 'relevance')} | "
              f"{f3(r, 'by_hand')} | {r['relevance_peak_gib']} / {r['by_hand_peak_gib']} | {r['max_diff_rel_to_max']:.1e} |")
    line = json.dumps({'relevance_bench': rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
