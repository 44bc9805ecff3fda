"""Throughput of BEiT's DiscreteVAE (discrete_vae_type = 'customized') on the HIP engine: images/s of
get_codebook_indices (images -> token ids) and of decode (token ids -> images) against the same structure run through
torch's own fp16 channels-last convolutions, on the same card, in the same process, interleaved (engine, torch, engine,
torch, ...: each round times both, so drift of the card hits both alike).

    python tools/custom_dvae_bench.py [--batch 64] [--size 112] [--rounds 9] [--iters 5] [--no-torch] [--layers]

Times are device events around `iters` calls, after a warm-up of both paths; reported: the median round and the spread
over the rounds.  `--layers` adds the two resampling kernels alone at the shapes this network gives them, each against
torch's convolution of the same shape.  Needs a GPU: there is no CPU fall-back.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from exploremultimodal_amd import dvae, hip, synth


class TorchVAE:
    """The same layers through torch: fp16 weights and activations, channels-last."""

    def __init__(self, vae):
        self.vae = vae
        self.half = {n: p.detach().half() for n, p in vae.named_parameters()}
        for n, p in self.half.items():
            if p.dim() == 4:
                self.half[n] = p.contiguous(memory_format=torch.channels_last)

    def _res(self, p, x):
        h = self.half
        t = F.relu(F.conv2d(x, h[p + '.net.0.weight'], h[p + '.net.0.bias'], padding=1))
        t = F.relu(F.conv2d(t, h[p + '.net.2.weight'], h[p + '.net.2.bias'], padding=1))
        return F.conv2d(t, h[p + '.net.4.weight'], h[p + '.net.4.bias']) + x

    @torch.no_grad()
    def indices(self, img):
        h, L = self.half, self.vae.num_layers
        x = img.half().contiguous(memory_format=torch.channels_last)
        for i in range(L):
            x = F.relu(F.conv2d(x, h[f'encoder.{2 * i}.0.weight'], h[f'encoder.{2 * i}.0.bias'], stride=2, padding=1))
            x = self._res(f'encoder.{2 * i + 1}', x)
        return F.conv2d(x, h[f'encoder.{2 * L}.weight'], h[f'encoder.{2 * L}.bias']).argmax(1)

    @torch.no_grad()
    def decode(self, ids):
        h, L = self.half, self.vae.num_layers
        B, n = ids.shape
        s = int(n ** 0.5)
        x = h['codebook.weight'][ids].view(B, s, s, -1).permute(0, 3, 1, 2)
        for i in range(L):
            x = F.relu(F.conv_transpose2d(x, h[f'decoder.{2 * i}.0.weight'], h[f'decoder.{2 * i}.0.bias'], stride=2,
                                          padding=1))
            x = self._res(f'decoder.{2 * i + 1}', x)
        return F.conv2d(x, h[f'decoder.{2 * L}.weight'], h[f'decoder.{2 * L}.bias']).float()


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def compare(tag, engine, torch_fn, rounds, iters, per=None):
    for _ in range(2):
        engine()
        if torch_fn is not None:
            torch_fn()
    te, tt = [], []
    for _ in range(rounds):
        te.append(timed(engine, iters))
        if torch_fn is not None:
            tt.append(timed(torch_fn, iters))
    me = statistics.median(te)
    unit = (lambda t: f' = {per / t:.0f} images/s') if per else (lambda t: '')
    line = f'{tag}: engine {me * 1e3:.3f} ms ({min(te) * 1e3:.3f} - {max(te) * 1e3:.3f}){unit(me)}'
    if tt:
        mt = statistics.median(tt)
        line += (f'; torch fp16 channels-last {mt * 1e3:.3f} ms ({min(tt) * 1e3:.3f} - {max(tt) * 1e3:.3f}){unit(mt)}; '
                 f'engine / torch = {mt / me:.2f}x')
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=112)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--layers', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('custom_dvae_bench needs a GPU')
    B, s = args.batch, args.size
    vae = dvae.DiscreteVAE(image_size=s, num_layers=3, num_tokens=8192, codebook_dim=512, hidden_dim=256)
    vae.load_state_dict(synth.synth_custom_dvae_state_dict(0), strict=True)
    vae = vae.cuda().eval()
    ref = None if args.no_torch else TorchVAE(vae)
    g = torch.Generator().manual_seed(s)
    img = torch.randn(B, 3, s, s, generator=g).cuda()
    ids = vae.get_codebook_indices(img).flatten(1)
    if ref is not None:
        try:
            agree = (ref.indices(img).flatten(1) == ids).float().mean().item()
            diff = (ref.decode(ids) - vae.decode(ids)).abs().max().item()
        except RuntimeError as e:                             # torch's convolution path cannot run on this box
            print(f'torch comparison not run: {type(e).__name__}: {str(e).splitlines()[0] if str(e) else ""}')
            ref = None
    if ref is not None:
        print(f'B={B} {s} px: ids equal to torch fp16 at {100 * agree:.2f} % of the positions; max |decode engine - torch| = '
              f'{diff:.3g}')
    compare(f'get_codebook_indices B={B} {s} px', lambda: vae.get_codebook_indices(img),
            None if ref is None else (lambda: ref.indices(img)), args.rounds, args.iters, per=B)
    compare(f'decode B={B} {s // 8}x{s // 8} tokens -> {s} px', lambda: vae.decode(ids),
            None if ref is None else (lambda: ref.decode(ids)), args.rounds, args.iters, per=B)
    if not args.layers:
        return
    f16 = torch.float16
    for h in (s // 2, s // 4):                                   # the two implicit down-convolutions (the stem is a GEMM)
        x = torch.randn(B, 256, h, h, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
        w = (torch.randn(256, 256, 4, 4, generator=g) / 64).half().cuda()
        xm = x.permute(0, 2, 3, 1).reshape(-1, 256)
        wq, wt = dvae.tap_major_shadow(w), w.contiguous(memory_format=torch.channels_last)
        out = torch.empty(B * h * h // 4, 256, dtype=f16, device='cuda')
        compare(f'conv4s2 B={B} {h}x{h} 256->256 ({2 * out.shape[0] * 256 * 4096 / 1e9:.1f} GFLOP)',
                lambda: hip.conv4s2_nhwc(xm, B, h, h, 256, wq, 256, out, relu=True),
                None if ref is None else (lambda: F.relu(F.conv2d(x, wt, stride=2, padding=1))), args.rounds, args.iters)
    for h, cin in ((s // 8, 512), (s // 4, 256), (s // 2, 256)):
        x = torch.randn(B, cin, h, h, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
        w = (torch.randn(cin, 256, 4, 4, generator=g) / 32).half().cuda()
        xm = x.permute(0, 2, 3, 1).reshape(-1, cin)
        wq, wt = dvae.convT4s2_shadow(w), w.contiguous(memory_format=torch.channels_last)
        out = torch.empty(B * h * h * 4, 256, dtype=f16, device='cuda')
        compare(f'convT4s2 B={B} {h}x{h} {cin}->256 ({2 * out.shape[0] * 256 * 4 * cin / 1e9:.1f} GFLOP)',
                lambda: hip.convT4s2_nhwc(xm, B, h, h, cin, wq, 256, out, relu=True),
                None if ref is None else (lambda: F.relu(F.conv_transpose2d(x, wt, stride=2, padding=1))), args.rounds,
                args.iters)


if __name__ == '__main__':
    main()
