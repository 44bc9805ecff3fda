"""dVAE decoder throughput: images/s of Dalle_VAE.decode (token ids -> [B, 6, H, W]) on the HIP engine against the same
Decoder structure run through torch's own fp16 channels-last convolutions, on the same card, in the same process,
interleaved (engine, torch, engine, torch, ...: each round times both, so drift of the card hits both alike).

    python tools/dvae_decode_bench.py [--batch 64] [--tokens 14 28] [--rounds 5] [--iters 5] [--no-torch]

Times are host clocks around `iters` calls that end in a device synchronise, after a warm-up of every shape; reported
per shape: the median round and the spread over the rounds.  FLOPs are counted from the layer shapes (2 * MACs of the
convolutions the reference runs, its upsampling order), so TFLOP/s is comparable between the two paths although the
engine's 1x1 convolutions after an upsampling do a quarter of that work.  Needs a GPU: there is no CPU fall-back.
`--no-torch` (for a kernel-trace run of the engine alone) skips the comparison.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from exploremultimodal_amd import dvae, synth


def reference_flops(dec, h, w):
    """2 * MACs per image of the decoder as the reference orders it (dall_e/decoder.py:75-124); the one-hot input
    convolution counts as a gather (0)."""
    total, hw = 0, h * w
    for g in range(1, 5):
        grp = getattr(dec.blocks, f'group_{g}')
        for bi in range(1, dec.n_blk_per_group + 1):
            blk = getattr(grp, f'block_{bi}')
            for m in [blk.id_path] + [getattr(blk.res_path, f'conv_{i}') for i in (1, 2, 3, 4)]:
                if isinstance(m, dvae.Conv2d):
                    total += 2 * hw * m.n_in * m.n_out * m.kw * m.kw
        if g < 4:
            hw *= 4
    oc = dec.blocks.output.conv
    return total + 2 * hw * oc.n_in * oc.n_out


class TorchDecoder:
    """The same structure through torch's convolutions: fp16 weights and activations, channels-last (what the reference
    runs on a GPU, dall_e/utils.py:37-41, with the memory format torch's ROCm convolutions prefer); the input layer as
    an embedding lookup, like the engine."""

    def __init__(self, dec):
        self.dec = dec
        cl = lambda t: t.half().contiguous(memory_format=torch.channels_last)
        self.w = {n: (cl(m.w.detach()), m.b.detach().half(), (m.kw - 1) // 2)
                  for n, m in dec.named_modules() if isinstance(m, dvae.Conv2d) and n != 'blocks.input'}
        self.table, self.bias = dec.blocks.input.shadow_embed()

    def conv(self, name, x):
        w, b, pad = self.w[name]
        return F.conv2d(x, w, b, padding=pad)

    @torch.no_grad()
    def __call__(self, ids):
        dec = self.dec
        x = (self.table[ids] + self.bias).half().permute(0, 3, 1, 2)        # [B, n_init, h, w], channels-last strides
        for g in range(1, 5):
            for bi in range(1, dec.n_blk_per_group + 1):
                p = f'blocks.group_{g}.block_{bi}'
                blk = getattr(getattr(dec.blocks, f'group_{g}'), f'block_{bi}')
                t = x
                for ci in (1, 2, 3, 4):
                    t = self.conv(f'{p}.res_path.conv_{ci}', F.relu(t))
                idp = self.conv(p + '.id_path', x) if isinstance(blk.id_path, dvae.Conv2d) else x
                x = idp + blk.post_gain * t
            if g < 4:
                x = F.interpolate(x, scale_factor=2, mode='nearest')
        return self.conv('blocks.output.conv', F.relu(x)).float()


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--tokens', type=int, nargs='+', default=[14, 28], help='token grid sides (14 -> 112 px, 28 -> 224 px)')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dvae_decode_bench needs a GPU')
    dec = dvae.Decoder()
    dec.load_state_dict(synth.synth_dvae_decoder_state_dict(0), strict=True)
    dec = dec.cuda()
    ref = None if args.no_torch else TorchDecoder(dec)
    B = args.batch
    for side in args.tokens:
        vae = dvae.Dalle_VAE(8 * side)
        vae.decoder = dec
        g = torch.Generator().manual_seed(side)
        ids = torch.randint(0, dec.vocab_size, (B, side * side), generator=g).cuda()
        grid = ids.view(B, side, side)
        flops = reference_flops(dec, side, side) * B
        tag = f'B={B} {side}x{side} tokens -> {8 * side} px'
        try:
            y = vae.decode(ids)                               # warm-up, and the outputs to compare
            torch_ok, why = ref is not None, 'skipped (--no-torch)'
            if ref is not None:
                try:
                    yt = ref(grid)
                    diff = (y - yt).abs().max().item()
                    del yt
                except Exception as e:                        # torch's convolution path cannot run on this box
                    torch_ok, why = False, f'{type(e).__name__}: {str(e).splitlines()[0] if str(e) else ""}'
            del y
            for _ in range(2):
                vae.decode(ids)
                if torch_ok:
                    ref(grid)
            te, tt = [], []
            for _ in range(args.rounds):
                te.append(timed(lambda: vae.decode(ids), args.iters))
                if torch_ok:
                    tt.append(timed(lambda: ref(grid), args.iters))
        except torch.OutOfMemoryError:
            print(f'{tag}: does not fit in device memory')
            torch.cuda.empty_cache()
            continue
        me = statistics.median(te)
        print(f'{tag}: engine {me * 1e3:.2f} ms ({min(te) * 1e3:.2f} - {max(te) * 1e3:.2f}) = {B / me:.0f} images/s, '
              f'{flops / me / 1e12:.0f} TFLOP/s of the reference\'s {flops / B / 1e9:.1f} GFLOP per image')
        if torch_ok:
            mt = statistics.median(tt)
            print(f'{tag}: torch fp16 channels-last {mt * 1e3:.2f} ms ({min(tt) * 1e3:.2f} - {max(tt) * 1e3:.2f}) = '
                  f'{B / mt:.0f} images/s; engine / torch = {mt / me:.2f}x; max |engine - torch| = {diff:.3g}')
        else:
            print(f'{tag}: torch comparison not run: {why}')


if __name__ == '__main__':
    main()
