"""Padded against variable-length text (VLMO.forward_features(txt_lens=...)) on one MI355X: forward + backward of the
VLMo-Base backbone, B = 64, 224 px, dropout / drop-path 0.1, in the image-text ('vl') and the text-only ('l') mode at
T = 64 and T = 40.

Lengths: a STAND-IN for caption lengths, not data -- len = min(T, 2 + round(exp(N(log 11, 0.35)))) per sample ([CLS] +
a log-normal word-piece count with median 11 + [SEP]; mean about 14), torch seed --seed.  The text mask is the prefix
mask of those lengths, so both variants compute the same function at the positions that exist.

Before timing the two variants are compared in eval mode on the timed shapes: outputs at the existing positions and
every parameter gradient of the loss (x * R * real).sum(); the tool stops if they differ by more than twice the
tolerances the tests hold either of them to against the fp32 oracle.  Timing: padded and ragged alternate in the same
process on the same batch, --warmup rounds first, device events around forward + backward, median and min - max of
--rounds (>= 7) rounds.  Also printed: the packed row counts and, per attention launch of the pass, its sequence count,
its maximum length and the form of the attention kernels that maximum selects (attention.hip: <= 256 tokens plain,
257 - 288 fringe, above streaming).

usage: python tools/ragged_text_bench.py [--batch 64] [--rounds 9] [--warmup 3] [--seed 0] [--T 64 40]"""
import argparse
import math
import os
import statistics
import sys
from functools import partial

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from exploremultimodal_amd import engine, synth
from exploremultimodal_amd.vlmo import VLMO, LayerNorm

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--rounds', type=int, default=9)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--seed', type=int, default=0)
ap.add_argument('--T', type=int, nargs='+', default=[64, 40])
ap.add_argument('--preset', default='base')
args = ap.parse_args()
if args.rounds < 7:
    ap.error('--rounds must be at least 7')
dev = torch.device('cuda:0')
B = args.batch


def form(maxlen):
    return 'plain (<= 256)' if maxlen <= 256 else ('fringe (257-288)' if maxlen <= 288 else 'streaming (> 288)')


def build(T):
    mc = synth.make_config(args.preset, max_text_len=T).model
    m = VLMO(img_size=mc.img_size, patch_size=mc.patch_size, in_chans=mc.in_chans, num_classes=mc.num_classes,
             embed_dim=mc.embed_dim, depth=mc.depth, num_heads=mc.num_heads, mlp_ratio=mc.mlp_ratio, qkv_bias=mc.qkv_bias,
             drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.1, norm_layer=partial(LayerNorm, eps=1e-12),
             init_values=mc.init_values, vocab_size=mc.vocab_size, max_text_len=T, fusion_layer=mc.fusion_layer)
    m.load_state_dict(synth.synth_backbone_state_dict(mc, 0, [('v', 'l', 'vl')] * mc.depth), strict=True)
    for b in m.blocks[:mc.fusion_layer]:          # pretrain layout: no 'vl' expert below the fusion layer
        del b.mlp['vl']
    return m.to(dev), mc


def fwd_bwd(model, kw, R, lens):
    for p in model.parameters():
        p.grad = None
    x, _ = model.forward_features(txt_lens=lens, **kw)
    (x * R).sum().backward()
    return x


for T in args.T:
    model, mc = build(T)
    P = synth.num_img_tokens(mc)
    g = torch.Generator().manual_seed(args.seed)
    words = torch.exp(torch.randn(B, generator=g) * 0.35 + math.log(11.0)).round().long()
    lens = tuple(int(n) for n in (words + 2).clamp(1, T))
    batch = synth.synth_batch(mc, B, seed=1234, pad=False, mim=False)
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).long()
    ids = batch['text_ids'] * mask
    im = torch.ones(B, P, dtype=torch.int64, device=dev)
    kws = {'vl': dict(img=batch['image'].to(dev), txt=ids.to(dev), img_attn_masks=im, txt_attn_masks=mask.to(dev)),
           'l': dict(txt=ids.to(dev), txt_attn_masks=mask.to(dev))}
    print(f'== {mc.name}  B = {B}  T = {T}  P = {P}  lengths: mean {sum(lens) / B:.1f}  min {min(lens)}  max {max(lens)}  '
          f'(seed {args.seed})')
    for mode, kw in kws.items():
        Pm = P if mode == 'vl' else 0
        real = mask if mode == 'l' else torch.cat([mask, torch.ones(B, P, dtype=torch.int64)], 1)
        R = (torch.randn(B, T + Pm, mc.embed_dim, generator=g) / 64.0 * real[..., None]).to(dev)
        for tag, ln in (('padded', None), ('ragged', lens)):
            pl = engine.Plan(B, T, Pm, 'cpu', mask, None, txt_lens=ln)
            seen = []
            for fused in ((False, True) if mode == 'vl' else (False,)):
                seen.append(('fused ' if fused else 'below fusion ' if mode == 'vl' else '') +
                            ', '.join(f'{n} seq max {ml}: {form(ml)}' for _, n, ml in pl.attn_launches(fused)))
            print(f'  {mode} {tag}: packed rows M = {pl.M} (text {pl.nt})  attention: ' + ' | '.join(seen))
        # ---- the two variants compute the same thing (eval mode: no dropout)
        model.eval()
        xp = fwd_bwd(model, kw, R, None).detach()
        gp = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        xr = fwd_bwd(model, kw, R, lens).detach()
        gr = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        keep = real.bool().to(dev)[..., None].expand_as(xp)
        assert bool((xr[~keep] == 0).all()), 'dropped rows are not 0'
        err = (xr - xp).abs()[keep]
        bound = 2 * (3e-2 + 2e-2 * xp.abs()[keep])
        worst = max(((gr[n] - gp[n]).norm().item() / (gp[n].norm().item() + 1e-12), n) for n in gp)
        print(f'  {mode} ragged vs padded (eval): out max |diff| {err.max().item():.5f} mean {err.mean().item():.6f}  '
              f'worst gradient {worst[0]:.4f} of its norm ({worst[1]})')
        if not bool((err <= bound).all()) or err.mean().item() > 8e-3 or worst[0] > 1e-1 or set(gp) != set(gr):
            sys.exit('the two variants disagree: not timed')
        # ---- timing
        model.train()
        times = {'padded': [], 'ragged': []}
        for r in range(args.warmup + args.rounds):
            for tag, ln in (('padded', None), ('ragged', lens)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fwd_bwd(model, kw, R, ln)
                e1.record()
                e1.synchronize()
                if r >= args.warmup:
                    times[tag].append(e0.elapsed_time(e1))
        med = {k: statistics.median(v) for k, v in times.items()}
        for tag in ('padded', 'ragged'):
            print(f'  {mode} {tag}: fwd+bwd median {med[tag]:.3f} ms  (min {min(times[tag]):.3f}  max {max(times[tag]):.3f}, '
                  f'{args.rounds} rounds)')
        print(f'  {mode} ragged / padded = {med["ragged"] / med["padded"]:.3f}')
    del model
    torch.cuda.empty_cache()
