"""Host-side mirror of the dall_e dVAE (encoder and decoder) and its VLMo wrapper.

Reference: dall_e/encoder.py:13-133 (EncoderBlock, Encoder), dall_e/decoder.py:13-136 (DecoderBlock, Decoder),
dall_e/utils.py:11-65 (Conv2d, map_pixels, unmap_pixels), models/modeling_discrete_vae.py:224-261 (Dalle_VAE),
models/vlmo/objectives.py:595-607 (create_d_vae / get_dalle_vae).

Same module tree (=> same state-dict keys: ``blocks.group_1.block_1.res_path.conv_1.w``),
constructor arguments, validators and ValueErrors; the arithmetic runs on the HIP engine:
NHWC fp16 activations (the reference runs this encoder in fp16 on GPU, utils.py:37-42),
3x3 convolutions as implicit MFMA GEMMs with bias+ReLU fused, the EncoderBlock tail
``id + post_gain * res`` fused into the 1x1 conv's epilogue, and for
``get_codebook_indices`` the 8192-way arg-max fused into the last 1x1 conv so the
[B, 8192, 14, 14] logits never reach HBM.

The decoder turns visual-token ids (or a [B, vocab, h, w] map of probabilities) back into the six logit-Laplace
parameter planes of an image: the input convolution on a one-hot map is a row gather (``Decoder.decode_ids``: the
[B, 8192, h, w] one-hot tensor never exists), the DecoderBlock tail ``id + post_gain * conv_4(...)`` is the residual
epilogue of the 3x3 convolution, the nearest-neighbour upsampling runs after the 1x1 convolutions of the block that
follows it, and the six-channel output head writes fp32 NCHW directly.  Inference only: no autograd.

``DiscreteVAE`` / ``ResBlock`` (models/modeling_discrete_vae.py:68-221) are BEiT's tokenizer, the reference's
``discrete_vae_type = 'customized'``: the same engine plus a 4x4 stride-2 convolution and transposed convolution of its
own (csrc/conv4s2.hip).
"""
import math
import os
from collections import OrderedDict

import torch
import torch.nn as nn

from . import derived, hip

logit_laplace_eps = 0.1
# measurement switch: 0 = the output convolution as one launch whatever its last dispatch round looks like
OUTPUT_ROW_SPLIT = os.environ.get('VLMO_DVAE_OUT_SPLIT', '1') != '0'


def _need_cuda(device):
    if device.type != 'cuda':
        raise RuntimeError('exploremultimodal_amd runs on MI355X only: input must be on a cuda (ROCm) device')


def _check_id_range(ids, vocab, name):
    """Token ids before a table lookup: not empty and, like the reference's F.one_hot, inside [0, vocab) (one
    device-to-host read)."""
    if ids.numel() == 0:
        raise ValueError(f'{name} is empty')
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= vocab:
        raise ValueError(f'ids must lie in [0, {vocab}): got values in [{lo}, {hi}]')


def _vocab_head(epi, feat, w, bias, N, parts, k1=0):
    """The vocabulary convolution (a plain GEMM) of feat fp16 [M, C] over the row ranges ``parts`` [(r0, r1, tile)]:
    EPI_F32 -> fp32 logits [M, N]; EPI_ARGMAX -> their arg-max per row, int64 [M], reduced from per-64-column partials
    so the logits never reach HBM.  ``k1`` > 0: w = [w_hi | w_lo] (Conv2d.shadow_split) as a two-segment reduction whose
    second segment reads the same activations (no doubled copy in HBM)."""
    M, dev = feat.shape[0], feat.device
    if epi == hip.EPI_ARGMAX:
        nchunk = (N + 63) // 64
        out, ldo = torch.empty((M, nchunk, 2), dtype=torch.float32, device=dev), nchunk
    else:
        out, ldo = torch.empty((M, N), dtype=torch.float32, device=dev), None
    for r0, r1, tile in parts:
        a = feat[r0:r1]
        hip.gemm_nt(epi, a, w, r1 - r0, N, w.shape[1], out[r0:r1], bias=bias, ldo=ldo, tile=tile,
                    A2=a if k1 else None, k1=k1)
    if epi != hip.EPI_ARGMAX:
        return out
    ids = torch.empty((M,), dtype=torch.int64, device=dev)
    hip.argmax_reduce(out, nchunk, ids, M)
    return ids


def map_pixels(x):
    """dall_e/utils.py:51-55."""
    if x.dtype != torch.float:
        raise ValueError('expected input to have type float')
    return (1 - 2 * logit_laplace_eps) * x + logit_laplace_eps


def unmap_pixels(x):
    """dall_e/utils.py:58-65."""
    if len(x.shape) != 4:
        raise ValueError('expected input to be 4d')
    if x.dtype != torch.float:
        raise ValueError('expected input to have type float')
    return torch.clamp((x - logit_laplace_eps) / (1 - 2 * logit_laplace_eps), 0, 1)


class Conv2d(nn.Module):
    """dall_e/utils.py:11-48 parameter container (w [n_out, n_in, kw, kw], b [n_out])."""

    def __init__(self, n_in, n_out, kw, use_float16=True, device=torch.device('cpu'), requires_grad=False):
        super().__init__()
        if n_in < 1 or n_out < 1 or kw < 1 or kw % 2 != 1:
            raise ValueError('Conv2d: need n_in >= 1, n_out >= 1, odd kw >= 1')
        self.n_in, self.n_out, self.kw, self.use_float16 = n_in, n_out, kw, use_float16
        w = torch.empty((n_out, n_in, kw, kw), dtype=torch.float32, device=device)
        w.normal_(std=1 / math.sqrt(n_in * kw ** 2))
        b = torch.zeros((n_out,), dtype=torch.float32, device=device)
        self.w = nn.Parameter(w, requires_grad=requires_grad)
        self.b = nn.Parameter(b, requires_grad=requires_grad)

    def _derived(self, slot, weight):
        """(``weight()``, fp32 bias), one slot per layout, each rebuilt when ``w`` or ``b`` was written to or moved."""
        return derived.of(self).get(slot, (self.w, self.b), lambda: (weight(), self.b.detach().float().contiguous()))

    def shadow_embed(self):
        """Decoder input layer (kw = 1, use_float16=False, dall_e/decoder.py:77-78) applied to a one-hot map: the fp32
        weight transposed to [n_in, n_out] = one row per token id, and the fp32 bias."""
        def table():
            if self.kw != 1:
                raise ValueError('shadow_embed: a 1x1 convolution only')
            return self.w.detach().float().reshape(self.n_out, self.n_in).t().contiguous()
        return self._derived('embed', table)

    def shadow_split(self):
        """use_float16=False layers (the output conv, dall_e/encoder.py:116-119 + dall_e/utils.py:37-48: fp32 weights
        on fp32 activations): the fp32 weight as TWO fp16 matrices side by side, [w_hi | w_lo] with w_hi = fp16(w) and
        w_lo = fp16(w - w_hi) (~22 significant bits together), multiplied against the activations repeated twice
        along K.  The fp16 MFMA products are exact in the fp32 accumulator, so the arg-max-deciding logits see the
        reference's weight precision, not a 11-bit rounding of it."""
        def split():
            w = self.w.detach().permute(0, 2, 3, 1).reshape(self.n_out, -1).float()
            hi = w.to(torch.float16)
            lo = (w - hi.float()).to(torch.float16)
            return torch.cat([hi, lo], 1).contiguous()
        return self._derived('split', split)

    def shadow(self):
        """fp16 weight in the engine's layout [n_out, kw*kw*n_in] (tap-major, channel-minor; the 3-channel
        stem keeps (c, ky, kx) order and is zero-padded to a multiple of 64 columns)."""
        def engine_layout():
            w = self.w.detach()
            if self.n_in % 64 == 0:
                s = w.permute(0, 2, 3, 1).reshape(self.n_out, -1)
            else:
                s = w.reshape(self.n_out, -1)
                pad = (-s.shape[1]) % 64
                s = torch.nn.functional.pad(s, (0, pad))
            return s.to(torch.float16).contiguous()
        return self._derived('shadow', engine_layout)


class EncoderBlock(nn.Module):
    """dall_e/encoder.py:13-46."""

    def __init__(self, n_in, n_out, n_layers, device=None, requires_grad=False):
        super().__init__()
        if n_in < 1 or n_out < 1 or n_out % 4 != 0 or n_layers < 1:
            raise ValueError('EncoderBlock: need n_in >= 1, n_out % 4 == 0, n_layers >= 1')
        self.n_in, self.n_out, self.n_layers = n_in, n_out, n_layers
        self.n_hid = n_out // 4
        self.post_gain = 1 / (n_layers ** 2)
        mk = lambda a, b, k: Conv2d(a, b, k, device=device or torch.device('cpu'), requires_grad=requires_grad)
        self.id_path = mk(n_in, n_out, 1) if n_in != n_out else nn.Identity()
        self.res_path = nn.Sequential(OrderedDict([
            ('relu_1', nn.ReLU()), ('conv_1', mk(n_in, self.n_hid, 3)),
            ('relu_2', nn.ReLU()), ('conv_2', mk(self.n_hid, self.n_hid, 3)),
            ('relu_3', nn.ReLU()), ('conv_3', mk(self.n_hid, self.n_hid, 3)),
            ('relu_4', nn.ReLU()), ('conv_4', mk(self.n_hid, n_out, 1))]))

    def tail_shadow(self):
        """Convolutional id_path: [conv_4.w | id_path.w] as ONE fp16 matrix [n_out, n_hid + n_in] and the combined bias
        post_gain * conv_4.b + id_path.b, for the block tail as a single two-segment GEMM (encoder.py:45-46)."""
        c4, idp = self.res_path.conv_4, self.id_path

        def tail():
            w4, b4 = c4.shadow()
            wi, bi = idp.shadow()
            return torch.cat([w4, wi], 1).contiguous(), (self.post_gain * b4 + bi).contiguous()
        return derived.of(self).get('tail', (c4.w, c4.b, idp.w, idp.b), tail)


class Encoder(nn.Module):
    """dall_e/encoder.py:49-133."""
    group_count = 4     # a class constant upstream (encoder.py:51): instances unpickled from encoder.pkl do not carry it

    def __init__(self, group_count=4, n_hid=256, n_blk_per_group=2, input_channels=3, vocab_size=8192,
                 device=torch.device('cpu'), requires_grad=False, use_mixed_precision=True):
        super().__init__()
        if n_hid < 64 or n_blk_per_group < 1 or input_channels < 1 or vocab_size < 512:
            raise ValueError('Encoder: n_hid >= 64, n_blk_per_group >= 1, input_channels >= 1, vocab_size >= 512')
        if group_count != 4:
            raise NotImplementedError('group_count is fixed to 4 in dall_e/encoder.py:51')
        self.group_count, self.n_hid, self.n_blk_per_group = group_count, n_hid, n_blk_per_group
        self.input_channels, self.vocab_size = input_channels, vocab_size
        self.use_mixed_precision = use_mixed_precision
        n_layers = group_count * n_blk_per_group
        mk = lambda a, b, k, **kw: Conv2d(a, b, k, device=device, requires_grad=requires_grad, **kw)
        blk = lambda a, b: EncoderBlock(a, b, n_layers=n_layers, device=device, requires_grad=requires_grad)
        groups = [('input', mk(input_channels, n_hid, 7))]
        prev = n_hid
        for g, mult in enumerate((1, 2, 4, 8)):
            items = [(f'block_{i + 1}', blk(prev if i == 0 else mult * n_hid, mult * n_hid))
                     for i in range(n_blk_per_group)]
            if g < 3:
                items.append(('pool', nn.MaxPool2d(kernel_size=2)))
            groups.append((f'group_{g + 1}', nn.Sequential(OrderedDict(items))))
            prev = mult * n_hid
        groups.append(('output', nn.Sequential(OrderedDict([
            ('relu', nn.ReLU()), ('conv', mk(8 * n_hid, vocab_size, 1, use_float16=False))]))))
        self.blocks = nn.Sequential(OrderedDict(groups))

    # ------------------------------------------------------------------ engine
    def _features(self, x):
        """-> relu(group_4 output) as fp16 [B*h*w, 8*n_hid], (B, h, w)."""
        if len(x.shape) != 4:
            raise ValueError(f'input shape {x.shape} is not 4d')
        if x.shape[1] != self.input_channels:
            raise ValueError(f'input has {x.shape[1]} channels but model built for {self.input_channels}')
        if x.dtype != torch.float32:
            raise ValueError('input must have dtype torch.float32')
        _need_cuda(x.device)
        if self.n_hid % 256 != 0:
            raise NotImplementedError('the implicit-GEMM kernels need n_hid to be a multiple of 256 '
                                      '(bottleneck width n_hid/4 must be a multiple of 64)')
        B, C, H, W = x.shape
        if H % 8 or W % 8:
            raise ValueError('image size must be a multiple of 8 (three 2x2 max-pools)')
        dev, f16 = x.device, torch.float16
        x = x.contiguous()
        em = lambda m, c: torch.empty((m, c), dtype=f16, device=dev)
        # stem 7x7 (encoder.py:75): explicit patches (3 input channels), raw + relu outputs
        stem = self.blocks.input
        ws, bs = stem.shadow()
        M = B * H * W
        cols = em(M, ws.shape[1])
        hip.dvae_im2col(x, cols, stem.kw, ws.shape[1])
        # only the raw feature map of every stage goes to HBM: the residual path's first convolution applies the ReLU to
        # its input fragments (relu_in), the identity path and the max-pool read the map as it is (encoder.py:21-29, 45-46)
        raw, rel = em(M, self.n_hid), None
        hip.gemm_nt(hip.EPI_DUAL, cols, ws, M, self.n_hid, ws.shape[1], raw, bias=bs, beta=1.0)
        del cols
        h, w = H, W
        for g in range(1, 5):
            grp = getattr(self.blocks, f'group_{g}')
            for bi in range(1, self.n_blk_per_group + 1):
                blk = getattr(grp, f'block_{bi}')
                hid, n_out = blk.n_hid, blk.n_out
                t = raw
                c_in = blk.n_in
                for ci in (1, 2, 3):
                    conv = getattr(blk.res_path, f'conv_{ci}')
                    wq, bq = conv.shadow()
                    o = em(M, hid)
                    hip.conv2d_nhwc(hip.EPI_BIAS, t, B, h, w, c_in, 3, wq, hid, o, bias=bq, relu=True, relu_in=(ci == 1))
                    t, c_in = o, hid
                last = g == 4 and bi == self.n_blk_per_group     # the output convolution (a plain GEMM) reads relu(x)
                raw2, rel2 = em(M, n_out), (em(M, n_out) if last else None)
                if isinstance(blk.id_path, Conv2d):
                    # id_path(x) + post_gain * conv_4(t) as ONE reduction over [t | x] against [conv_4.w | id_path.w]: the
                    # partial sum of the first segment takes post_gain in fp32 inside the kernel; no id-path tensor in HBM
                    wc, bc = blk.tail_shadow()
                    hip.gemm_nt(hip.EPI_DUAL, t, wc, M, n_out, hid + blk.n_in, raw2, out2=rel2, bias=bc, beta=1.0,
                                A2=raw, k1=hid, seg_scale=blk.post_gain)
                else:
                    w4, b4 = blk.res_path.conv_4.shadow()
                    hip.gemm_nt(hip.EPI_DUAL, t, w4, M, n_out, hid, raw2, out2=rel2, bias=b4, resid=raw,
                                beta=blk.post_gain)
                raw, rel = raw2, rel2
            if g < 4:
                C2 = raw.shape[1]
                Mp = B * (h // 2) * (w // 2)
                rp = em(Mp, C2)
                hip.maxpool2_nhwc(raw, rp, None, B, h, w, C2)
                raw, rel, h, w, M = rp, None, h // 2, w // 2, Mp
        return rel, (B, h, w)

    @staticmethod
    def _row_parts(M, N):
        """Row ranges [(r0, r1, tile)] of the output convolution.  Its 256 x 256 tiles run one per CU, so a last dispatch
        round that is mostly empty costs a whole round (64 images of 112 x 112: 49 x 32 = 1 568 tiles = 6.125 rounds of 256
        CUs, paid as 7): the rows of that round go out as a second launch of 128 x 128 tiles instead."""
        nt, rt = -(-N // 256), -(-M // 256)
        full, left = divmod(rt * nt, 256)
        if not OUTPUT_ROW_SPLIT or full == 0 or left == 0 or left > 64:
            return [(0, M, -1)]
        r = (full * 256 // nt) * 256
        return [(0, r, 3), (r, M, 0)] if 0 < r < M else [(0, M, -1)]

    def _head(self, epi, x):
        """[x | x] against [w_hi | w_lo] of the output convolution, over its row parts."""
        rel, dims = self._features(x)
        wo, bo = self.blocks.output.conv.shadow_split()
        M, C = rel.shape
        return _vocab_head(epi, rel, wo, bo, self.vocab_size, self._row_parts(M, self.vocab_size), k1=C), dims

    def forward(self, x):
        """encoder.py:123-133 -> logits fp32 [B, vocab, H/8, W/8]."""
        logits, (B, h, w) = self._head(hip.EPI_F32, x)
        return logits.view(B, h, w, self.vocab_size).permute(0, 3, 1, 2)

    def codebook_indices(self, x):
        """argmax(forward(x), dim=1) without materialising the logits -> int64 [B, H/8, W/8]."""
        ids, dims = self._head(hip.EPI_ARGMAX, x)
        return ids.view(dims)


class DecoderBlock(nn.Module):
    """dall_e/decoder.py:13-46: the 1x1 convolution comes first and conv_4 is a 3x3 to n_out channels."""

    def __init__(self, n_in, n_out, n_layers, device=None, requires_grad=False):
        super().__init__()
        if n_in < 1 or n_out < 1 or n_out % 4 != 0 or n_layers < 1:
            raise ValueError('DecoderBlock: need n_in >= 1, n_out % 4 == 0, n_layers >= 1')
        self.n_in, self.n_out, self.n_layers = n_in, n_out, n_layers
        self.n_hid = n_out // 4
        self.post_gain = 1 / (n_layers ** 2)
        mk = lambda a, b, k: Conv2d(a, b, k, device=device or torch.device('cpu'), requires_grad=requires_grad)
        self.id_path = mk(n_in, n_out, 1) if n_in != n_out else nn.Identity()
        self.res_path = nn.Sequential(OrderedDict([
            ('relu_1', nn.ReLU()), ('conv_1', mk(n_in, self.n_hid, 1)),
            ('relu_2', nn.ReLU()), ('conv_2', mk(self.n_hid, self.n_hid, 3)),
            ('relu_3', nn.ReLU()), ('conv_3', mk(self.n_hid, self.n_hid, 3)),
            ('relu_4', nn.ReLU()), ('conv_4', mk(self.n_hid, n_out, 3))]))


class Decoder(nn.Module):
    """dall_e/decoder.py:49-136.

    Order of operations: the reference upsamples at the END of groups 1-3 (decoder.py:85, 95, 105), so block_1 of the
    next group runs its id_path (decoder.py:30-32) and relu_1 -> conv_1 -> relu_2 (decoder.py:35-37) on the upsampled
    map.  A 1x1 convolution and a ReLU act per pixel and nearest-neighbour upsampling only repeats pixels, so they
    commute: here block_1 of groups 2-4 computes those two results on the map BEFORE the upsampling and upsamples them
    (n_out + n_out/4 channels instead of n_in = 2 n_out; the 1x1 convolutions run on a quarter of the pixels).  Every
    output pixel is the same products summed in the same order as in the reference's order.
    """
    group_count = 4     # a class constant upstream (decoder.py:51): instances unpickled from decoder.pkl do not carry it

    def __init__(self, group_count=4, n_init=128, n_hid=256, n_blk_per_group=2, output_channels=3, vocab_size=8192,
                 device=torch.device('cpu'), requires_grad=False, use_mixed_precision=True):
        super().__init__()
        if n_init < 8 or n_hid < 64 or n_blk_per_group < 1 or output_channels < 1 or vocab_size < 512:
            raise ValueError('Decoder: n_init >= 8, n_hid >= 64, n_blk_per_group >= 1, output_channels >= 1, '
                             'vocab_size >= 512')
        if group_count != 4:
            raise NotImplementedError('group_count is fixed to 4 in dall_e/decoder.py:51')
        self.group_count, self.n_init, self.n_hid, self.n_blk_per_group = group_count, n_init, n_hid, n_blk_per_group
        self.output_channels, self.vocab_size = output_channels, vocab_size
        self.use_mixed_precision = use_mixed_precision
        n_layers = group_count * n_blk_per_group
        mk = lambda a, b, k, **kw: Conv2d(a, b, k, device=device, requires_grad=requires_grad, **kw)
        blk = lambda a, b: DecoderBlock(a, b, n_layers=n_layers, device=device, requires_grad=requires_grad)
        groups = [('input', mk(vocab_size, n_init, 1, use_float16=False))]
        prev = n_init
        for g, mult in enumerate((8, 4, 2, 1)):
            items = [(f'block_{i + 1}', blk(prev if i == 0 else mult * n_hid, mult * n_hid))
                     for i in range(n_blk_per_group)]
            if g < 3:
                items.append(('upsample', nn.Upsample(scale_factor=2, mode='nearest')))
            groups.append((f'group_{g + 1}', nn.Sequential(OrderedDict(items))))
            prev = mult * n_hid
        groups.append(('output', nn.Sequential(OrderedDict([
            ('relu', nn.ReLU()), ('conv', mk(n_hid, 2 * output_channels, 1))]))))
        self.blocks = nn.Sequential(OrderedDict(groups))

    # ------------------------------------------------------------------ engine
    def _check_engine(self, device):
        _need_cuda(device)
        if self.n_hid % 256 != 0:
            raise NotImplementedError('the implicit-GEMM kernels need n_hid to be a multiple of 256 '
                                      '(bottleneck width n_hid/4 must be a multiple of 64)')
        if self.n_init % 64 != 0:
            raise NotImplementedError('the implicit-GEMM kernels need n_init to be a multiple of 64')
        if 2 * self.output_channels > 8:
            raise NotImplementedError('the output head holds at most 8 channels (output_channels <= 4)')

    def _body(self, raw, B, h, w):
        """raw = input-convolution output fp16 [B*h*w, n_init] -> fp32 [B, 2*output_channels, 8h, 8w]
        (decoder.py:79-123)."""
        dev, f16 = raw.device, torch.float16
        em = lambda m, c: torch.empty((m, c), dtype=f16, device=dev)
        M = B * h * w
        for g in range(1, 5):
            grp = getattr(self.blocks, f'group_{g}')
            for bi in range(1, self.n_blk_per_group + 1):
                blk = getattr(grp, f'block_{bi}')
                hid, n_out = blk.n_hid, blk.n_out
                # the identity path and the residual path's 1x1 convolution read the block's input: raw for the identity
                # path, relu(raw) applied to the input fragments for conv_1 (only raw maps go to HBM)
                if isinstance(blk.id_path, Conv2d):
                    wi, bi_ = blk.id_path.shadow()
                    idp = em(M, n_out)
                    hip.conv2d_nhwc(hip.EPI_BIAS, raw, B, h, w, blk.n_in, 1, wi, n_out, idp, bias=bi_)
                else:
                    idp = raw
                w1, b1 = blk.res_path.conv_1.shadow()
                t = em(M, hid)
                hip.conv2d_nhwc(hip.EPI_BIAS, raw, B, h, w, blk.n_in, 1, w1, hid, t, bias=b1, relu=True, relu_in=True)
                if g > 1 and bi == 1:
                    # the previous group's upsampling, moved behind this block's two 1x1 convolutions (class docstring)
                    idp2, t2 = em(4 * M, n_out), em(4 * M, hid)
                    hip.upsample2_nhwc(idp, idp2, B, h, w, n_out)
                    hip.upsample2_nhwc(t, t2, B, h, w, hid)
                    idp, t, h, w, M = idp2, t2, 2 * h, 2 * w, 4 * M
                for ci in (2, 3):
                    wq, bq = getattr(blk.res_path, f'conv_{ci}').shadow()
                    o = em(M, hid)
                    hip.conv2d_nhwc(hip.EPI_BIAS, t, B, h, w, hid, 3, wq, hid, o, bias=bq, relu=True)
                    t = o
                # id + post_gain * conv_4(t) (decoder.py:45-46) in the 3x3 convolution's epilogue, rounded to fp16 once
                w4, b4 = blk.res_path.conv_4.shadow()
                raw = em(M, n_out)
                hip.conv2d_nhwc(hip.EPI_DUAL, t, B, h, w, hid, 3, w4, n_out, raw, bias=b4, resid=idp, beta=blk.post_gain)
        wo, bo = self.blocks.output.conv.shadow()
        out = torch.empty((B, 2 * self.output_channels, h, w), dtype=torch.float32, device=dev)
        hip.dvae_out_head(raw, wo, bo, out, B, h, w)
        return out

    @torch.no_grad()
    def decode_ids(self, ids):
        """Visual-token ids int64 [B, h, w] -> fp32 [B, 2*output_channels, 8h, 8w]: ``forward`` of the one-hot map of
        ``ids`` (modeling_discrete_vae.py:241-244) without building it.  The ids are checked on the host (one
        device-to-host read): like the reference's F.one_hot, an id outside [0, vocab_size) raises."""
        if ids.dim() != 3:
            raise ValueError(f'ids shape {tuple(ids.shape)} is not [B, h, w]')
        if ids.dtype != torch.int64:
            raise ValueError('ids must have dtype torch.int64')
        self._check_engine(ids.device)
        B, h, w = ids.shape
        _check_id_range(ids, self.vocab_size, 'ids')
        table, bias = self.blocks.input.shadow_embed()
        raw = torch.empty((B * h * w, self.n_init), dtype=torch.float16, device=ids.device)
        hip.dvae_embed(ids.contiguous().view(-1), table, bias, raw)
        return self._body(raw, B, h, w)

    @torch.no_grad()
    def forward(self, x):
        """decoder.py:126-136: x fp32 [B, vocab, h, w] (probabilities or a one-hot map) -> fp32
        [B, 2*output_channels, 8h, 8w].  The input convolution (fp32 upstream, use_float16=False) runs as one MFMA GEMM
        with the fp32 weight split into two fp16 matrices [w_hi | w_lo] (Conv2d.shadow_split) against x ROUNDED TO FP16:
        exact for a one-hot map, a relative 2^-11 rounding of each probability otherwise."""
        if len(x.shape) != 4:
            raise ValueError(f'input shape {x.shape} is not 4d')
        if x.shape[1] != self.vocab_size:
            raise ValueError(f'input has {x.shape[1]} channels but model built for {self.vocab_size}')
        if x.dtype != torch.float32:
            raise ValueError('input must have dtype torch.float32')
        self._check_engine(x.device)
        if self.vocab_size % 64 != 0:
            raise NotImplementedError('the dense input convolution needs vocab_size to be a multiple of 64')
        B, V, h, w = x.shape
        M = B * h * w
        z = x.permute(0, 2, 3, 1).reshape(M, V).to(torch.float16)
        wi, bi = self.blocks.input.shadow_split()
        raw = torch.empty((M, self.n_init), dtype=torch.float16, device=x.device)
        hip.gemm_nt(hip.EPI_BIAS, z, wi, M, self.n_init, 2 * V, raw, bias=bi, A2=z, k1=V)
        return self._body(raw, B, h, w)


def load_model(path, device=None):
    """dall_e/__init__.py:12-21 for local files (the reference's http(s) branch needs network access and is
    not provided).  The OpenAI pickles reference classes ``dall_e.encoder.Encoder`` / ``dall_e.decoder.Decoder`` /
    ``dall_e.utils.Conv2d``: they are resolved to this module's mirrors while unpickling."""
    if path.startswith('http://') or path.startswith('https://'):
        raise NotImplementedError('remote dVAE weights are not fetched; download encoder.pkl / decoder.pkl and pass a local path')
    import sys
    import types
    fake = {}
    for name in ('dall_e', 'dall_e.encoder', 'dall_e.decoder', 'dall_e.utils'):
        if name not in sys.modules:
            fake[name] = types.ModuleType(name)
    for m in fake.values():
        m.Encoder, m.EncoderBlock, m.Conv2d = Encoder, EncoderBlock, Conv2d
        m.Decoder, m.DecoderBlock = Decoder, DecoderBlock
    sys.modules.update(fake)
    try:
        with open(path, 'rb') as f:
            enc = torch.load(f, map_location=device, weights_only=False)
    finally:
        for name in fake:
            sys.modules.pop(name, None)
    return enc


class Dalle_VAE(nn.Module):
    """models/modeling_discrete_vae.py:224-261.  The decoder is optional: pretraining only tokenises."""

    def __init__(self, image_size):
        super().__init__()
        self.encoder = None
        self.decoder = None
        self.image_size = image_size

    def load_model(self, model_dir, device):
        """modeling_discrete_vae.py:232-236; ``decoder.pkl`` is loaded when the directory has one."""
        self.encoder = load_model(os.path.join(model_dir, 'encoder.pkl'), device)
        dec = os.path.join(model_dir, 'decoder.pkl')
        self.decoder = load_model(dec, device) if os.path.exists(dec) else None

    def get_codebook_indices(self, images):
        return self.encoder.codebook_indices(images)

    def get_codebook_probs(self, images):
        return nn.Softmax(dim=1)(self.encoder(images))

    def _need_decoder(self):
        if self.decoder is None:
            raise RuntimeError('this Dalle_VAE has no decoder: put decoder.pkl next to encoder.pkl in the weight '
                               'directory, or build one with create_d_vae(..., with_decoder=True)')
        return self.decoder

    def _vocab(self):
        return self.encoder.vocab_size if self.encoder is not None else self.decoder.vocab_size

    def decode(self, img_seq):
        """modeling_discrete_vae.py:238-244: token ids [B, (image_size/8)^2] (any shape with that many per image) ->
        fp32 [B, 6, image_size, image_size], without the one-hot tensor."""
        dec = self._need_decoder()
        bsz = img_seq.size()[0]
        img_seq = img_seq.view(bsz, self.image_size // 8, self.image_size // 8)
        return dec.decode_ids(img_seq).float()

    def forward(self, img_seq_prob, no_process=False):
        """modeling_discrete_vae.py:254-261: probabilities [B, seq, vocab] (or, with no_process, [B, vocab, h, w])."""
        dec = self._need_decoder()
        if no_process:
            return dec(img_seq_prob.float()).float()
        bsz, seq_len, num_class = img_seq_prob.size()
        z = img_seq_prob.view(bsz, self.image_size // 8, self.image_size // 8, self._vocab())
        return dec(z.permute(0, 3, 1, 2).float()).float()


# ---------------------------------------------------------------------------------------------------------------------
# BEiT's DiscreteVAE (config.train.discrete_vae_type = 'customized'): models/modeling_discrete_vae.py:68-221

def tap_major_shadow(w):
    """Conv2d weight [Cout, Cin, k, k] -> fp16 [Cout, k*k*Cin], tap-major (k ky + kx), channel-minor: the layout of
    vlmo_conv2d_nhwc, vlmo_conv4s2_nhwc and (k = 1) a plain GEMM."""
    return w.detach().permute(0, 2, 3, 1).reshape(w.shape[0], -1).to(torch.float16).contiguous()


def convT4s2_shadow(w, cin_pad=None):
    """ConvTranspose2d(4, stride 2, padding 1) weight [Cin, Cout, 4, 4] -> fp16 [4, Cout, 4*Cin_pad]: quarter p = 2 py + px
    serves the output pixels of parity (py, px); its column (2 a + b) * Cin_pad + c holds w[c, n, 1 - py + 2 a,
    1 - px + 2 b], the tap that input pixel (y + py - a, x + px - b) contributes to output (2 y + py, 2 x + px).
    cin_pad > Cin adds zero columns (an input whose channel count is padded to a multiple of 64)."""
    cin, cout = w.shape[:2]
    cp = cin_pad or cin
    s = torch.zeros((4, cout, 4, cp), dtype=torch.float16, device=w.device)
    wd = w.detach()
    for py in (0, 1):
        for px in (0, 1):
            for a in (0, 1):
                for b in (0, 1):
                    s[2 * py + px, :, 2 * a + b, :cin] = wd[:, :, 1 - py + 2 * a, 1 - px + 2 * b].t().to(torch.float16)
    return s.reshape(4, cout, 4 * cp).contiguous()


def _conv_shadow(conv, build=None):
    """(fp16 engine-layout weight, fp32 bias) of an nn.Conv2d / nn.ConvTranspose2d; ``build`` makes the weight where
    it is not the tap-major one."""
    if build is None:
        build = lambda: tap_major_shadow(conv.weight)
    return derived.of(conv).get('shadow', (conv.weight, conv.bias),
                                lambda: (build(), conv.bias.detach().float().contiguous()))


class ResBlock(nn.Module):
    """modeling_discrete_vae.py:68-78: 3x3 + ReLU, 3x3 + ReLU, 1x1, plus the input."""

    def __init__(self, chan_in, hidden_size, chan_out):
        super().__init__()
        self.net = nn.Sequential(nn.Conv2d(chan_in, hidden_size, 3, padding=1), nn.ReLU(),
                                 nn.Conv2d(hidden_size, hidden_size, 3, padding=1), nn.ReLU(),
                                 nn.Conv2d(hidden_size, chan_out, 1))

    def run(self, x, B, h, w):
        """x fp16 [B*h*w, C] -> net(x) + x; the sum is the 1x1 convolution's residual epilogue, rounded to fp16 once."""
        c = x.shape[1]
        M = B * h * w
        t = x
        for i in (0, 2):
            wq, bq = _conv_shadow(self.net[i])
            o = torch.empty((M, c), dtype=torch.float16, device=x.device)
            hip.conv2d_nhwc(hip.EPI_BIAS, t, B, h, w, c, 3, wq, c, o, bias=bq, relu=True)
            t = o
        w4, b4 = _conv_shadow(self.net[4])
        out = torch.empty((M, c), dtype=torch.float16, device=x.device)
        hip.gemm_nt(hip.EPI_DUAL, t, w4, M, c, c, out, bias=b4, resid=x, beta=1.0)
        return out


class DiscreteVAE(nn.Module):
    """modeling_discrete_vae.py:81-221 with the reference's module tree (=> its state-dict keys: ``codebook.weight``,
    ``encoder.{2i}.0.*``, ``encoder.{2i+1}.net.{0,2,4}.*``, ``encoder.{2L}.*`` and the same under ``decoder.``) as a
    parameter container; tokenising and decoding run on the HIP engine in fp16 NHWC.  Inference only (eval semantics, no
    autograd): the Gumbel-softmax training pass of the tokenizer itself is not provided."""

    def __init__(self, image_size=256, num_tokens=512, codebook_dim=512, num_layers=3, hidden_dim=64, channels=3,
                 smooth_l1_loss=False, temperature=0.9, straight_through=False, kl_div_loss_weight=0.):
        super().__init__()
        if num_layers < 1:
            raise ValueError('DiscreteVAE: number of layers must be greater than or equal to 1')
        if hidden_dim < 64 or hidden_dim % 64 != 0:
            raise NotImplementedError(f'DiscreteVAE: the implicit-GEMM kernels need hidden_dim to be a multiple of 64 '
                                      f'(got {hidden_dim})')
        if num_tokens < 64 or num_tokens % 64 != 0:
            raise NotImplementedError(f'DiscreteVAE: the fused arg-max reduces 64-token chunks: num_tokens must be a '
                                      f'multiple of 64 (got {num_tokens})')
        if codebook_dim < 8 or codebook_dim % 8 != 0:
            raise NotImplementedError(f'DiscreteVAE: the codebook lookup moves 8 channels per thread: codebook_dim must '
                                      f'be a multiple of 8 (got {codebook_dim})')
        if channels != 3:
            raise NotImplementedError(f'DiscreteVAE: RGB images only (channels == 3, got {channels})')
        if image_size < 2 ** num_layers or image_size % 2 ** num_layers != 0:
            raise NotImplementedError(f'DiscreteVAE: image_size must be a multiple of 2**num_layers = {2 ** num_layers} '
                                      f'(got {image_size})')
        self.image_size, self.num_tokens, self.num_layers = image_size, num_tokens, num_layers
        self.codebook_dim, self.hidden_dim, self.channels = codebook_dim, hidden_dim, channels
        self.temperature, self.straight_through = temperature, straight_through
        self.smooth_l1_loss, self.kl_div_loss_weight = smooth_l1_loss, kl_div_loss_weight
        self.codebook = nn.Embedding(num_tokens, codebook_dim)
        enc, dec = [], []
        enc_in, dec_in = channels, codebook_dim
        for _ in range(num_layers):
            enc.append(nn.Sequential(nn.Conv2d(enc_in, hidden_dim, 4, stride=2, padding=1), nn.ReLU()))
            enc.append(ResBlock(hidden_dim, hidden_dim, hidden_dim))
            dec.append(nn.Sequential(nn.ConvTranspose2d(dec_in, hidden_dim, 4, stride=2, padding=1), nn.ReLU()))
            dec.append(ResBlock(hidden_dim, hidden_dim, hidden_dim))
            enc_in = dec_in = hidden_dim
        enc.append(nn.Conv2d(hidden_dim, num_tokens, 1))
        dec.append(nn.Conv2d(hidden_dim, channels, 1))
        self.encoder = nn.Sequential(*enc)
        self.decoder = nn.Sequential(*dec)

    def get_image_size(self):
        return self.image_size

    def get_image_tokens_size(self):
        return self.image_size // 8

    # ------------------------------------------------------------------ engine
    def _features(self, img):
        """-> the last ResBlock's output fp16 [B*h*w, hidden_dim], (B, h, w) with h = w = image_size / 2**num_layers."""
        if img.dim() != 4 or img.shape[1] != self.channels:
            raise ValueError(f'input shape {tuple(img.shape)} is not [B, {self.channels}, H, W]')
        if img.shape[-1] != self.image_size or img.shape[-2] != self.image_size:
            raise ValueError(f'input must have the correct image size {self.image_size}')
        if img.dtype != torch.float32:
            raise ValueError('input must have dtype torch.float32')
        _need_cuda(img.device)
        B, dev, hid = img.shape[0], img.device, self.hidden_dim
        h = w = self.image_size
        x = img.contiguous()
        t = None
        for li in range(self.num_layers):
            conv = self.encoder[2 * li][0]
            M = B * (h // 2) * (w // 2)
            o = torch.empty((M, hid), dtype=torch.float16, device=dev)
            if li == 0:
                # stem (3 input channels): explicit 4x4 stride-2 patches, K = 48 padded to 64, then a plain GEMM
                ws, bs = _conv_shadow(conv, lambda: nn.functional.pad(
                    conv.weight.detach().reshape(hid, -1), (0, 64 - 16 * self.channels)).to(torch.float16).contiguous())
                cols = torch.empty((M, 64), dtype=torch.float16, device=dev)
                hip.dvae_patch4s2(x, cols, 64)
                hip.gemm_nt(hip.EPI_BIAS, cols, ws, M, hid, 64, o, bias=bs, relu=True)
            else:
                wq, bq = _conv_shadow(conv)
                hip.conv4s2_nhwc(t, B, h, w, hid, wq, hid, o, bias=bq, relu=True)
            h, w = h // 2, w // 2
            t = self.encoder[2 * li + 1].run(o, B, h, w)
        return t, (B, h, w)

    def _head(self, epi, img):
        """The vocabulary convolution (1x1, hidden_dim -> num_tokens) on the features, as one launch."""
        feat, dims = self._features(img)
        wl, bl = _conv_shadow(self.encoder[2 * self.num_layers])
        return _vocab_head(epi, feat, wl, bl, self.num_tokens, [(0, feat.shape[0], -1)]), dims

    @torch.no_grad()
    def forward(self, img, return_loss=False, return_recons=False, return_logits=False, temp=None):
        """modeling_discrete_vae.py:171-184 with return_logits=True -> fp32 logits [B, num_tokens, h, w]."""
        if not return_logits:
            raise NotImplementedError('DiscreteVAE.forward without return_logits is the Gumbel-softmax training pass of the '
                                      'tokenizer itself (modeling_discrete_vae.py:186-221): this engine only tokenises '
                                      '(get_codebook_indices, forward(..., return_logits=True)) and decodes (decode)')
        logits, (B, h, w) = self._head(hip.EPI_F32, img)
        return logits.view(B, h, w, self.num_tokens).permute(0, 3, 1, 2)

    @torch.no_grad()
    def get_codebook_indices(self, images):
        """argmax(forward(images, return_logits=True), dim=1) -> int64 [B, h, w] with the arg-max fused into the
        vocabulary convolution: the [B, num_tokens, h, w] logits never exist."""
        ids, dims = self._head(hip.EPI_ARGMAX, images)
        return ids.view(dims)

    @torch.no_grad()
    def get_codebook_probs(self, images):
        return nn.Softmax(dim=1)(self.forward(images, return_logits=True))

    def _codebook_table(self):
        """fp32 codebook padded with zero columns to a multiple of 64 (the first transposed convolution's K chunks), and
        the zero bias of the lookup kernel."""
        cb = self.codebook.weight
        dp = -(-self.codebook_dim // 64) * 64
        return derived.of(self.codebook).get('table', (cb,), lambda: (
            nn.functional.pad(cb.detach().float(), (0, dp - self.codebook_dim)).contiguous(),
            torch.zeros(dp, dtype=torch.float32, device=cb.device)))

    @torch.no_grad()
    def decode(self, img_seq):
        """modeling_discrete_vae.py:162-169: token ids int64 [B, n] (n a square) -> fp32 [B, channels, s, s] with
        s = sqrt(n) * 2**num_layers.  Like ``Decoder.decode_ids`` an id outside [0, num_tokens) raises (one
        device-to-host read)."""
        if img_seq.dim() != 2:
            raise ValueError(f'img_seq shape {tuple(img_seq.shape)} is not [B, n]')
        if img_seq.dtype != torch.int64:
            raise ValueError('img_seq must have dtype torch.int64')
        _need_cuda(img_seq.device)
        B, n = img_seq.shape
        h = w = math.isqrt(n)
        if n == 0 or h * w != n:
            raise ValueError(f'img_seq holds {n} ids per image, which is not a square grid')
        _check_id_range(img_seq, self.num_tokens, 'img_seq')
        dev, hid = img_seq.device, self.hidden_dim
        table, zbias = self._codebook_table()
        cin = table.shape[1]
        t = torch.empty((B * n, cin), dtype=torch.float16, device=dev)
        hip.dvae_embed(img_seq.contiguous().view(-1), table, zbias, t)
        for li in range(self.num_layers):
            conv = self.decoder[2 * li][0]
            wq, bq = _conv_shadow(conv, lambda: convT4s2_shadow(conv.weight, cin))
            o = torch.empty((B * 4 * h * w, hid), dtype=torch.float16, device=dev)
            hip.convT4s2_nhwc(t, B, h, w, cin, wq, hid, o, bias=bq, relu=True)
            h, w, cin = 2 * h, 2 * w, hid
            t = self.decoder[2 * li + 1].run(o, B, h, w)
        wo, bo = _conv_shadow(self.decoder[2 * self.num_layers])
        out = torch.empty((B, self.channels, h, w), dtype=torch.float32, device=dev)
        hip.dvae_out_head_linear(t, wo, bo, out, B, h, w)
        return out


def create_d_vae(weight_path, d_vae_type, image_size, device, vocab_size=None, with_decoder=False):
    """objectives.py:595-628.  'dall-e': weight_path=None builds a randomly initialised encoder (synthetic runs) and, with
    with_decoder=True, a randomly initialised decoder (44 M parameters that a pretraining model does not need: off by
    default).  With a weight_path the decoder comes from <weight_path>/decoder.pkl when that file exists.
    'customized' (get_d_vae, objectives.py:610-628): BEiT's DiscreteVAE with 3 layers, 8192 tokens, codebook width 512,
    hidden width 256, loaded from <weight_path>/pytorch_model.bin['weights'].  The reference has no 'customized'
    tokenizer without weights (get_d_vae joins the path unconditionally); weight_path=None WITH an explicit ``vocab_size``
    builds a randomly initialised one of that many tokens for synthetic runs, and without one it is refused: that
    call asks for the reference's tokenizer and names no weights to load.  ``vocab_size`` defaults to 8192 for 'dall-e'."""
    if d_vae_type == 'dall-e':
        vae = Dalle_VAE(image_size)
        if vocab_size is None:
            vocab_size = 8192
        if weight_path is None:
            vae.encoder = Encoder(device=torch.device(device), vocab_size=vocab_size)
            if with_decoder:
                vae.decoder = Decoder(device=torch.device(device), vocab_size=vocab_size)
        else:
            vae.load_model(model_dir=weight_path, device=device)
        return vae
    if d_vae_type == 'customized':
        if weight_path is None:
            if vocab_size is None:
                raise NotImplementedError("create_d_vae(None, 'customized', ...): the customized tokenizer is loaded from "
                                          "<weight_path>/pytorch_model.bin; without a weight_path pass vocab_size=... for "
                                          'a randomly initialised one (synthetic runs)')
            return DiscreteVAE(image_size=image_size, num_layers=3, num_tokens=vocab_size, codebook_dim=512,
                               hidden_dim=256).to(device)
        state_dict = torch.load(os.path.join(weight_path, 'pytorch_model.bin'), map_location='cpu')['weights']
        model = DiscreteVAE(image_size=image_size, num_layers=3, num_tokens=8192, codebook_dim=512,
                            hidden_dim=256).to(device)
        model.load_state_dict(state_dict)
        return model
    raise NotImplementedError(f"discrete_vae_type {d_vae_type!r} is not one of 'dall-e', 'customized' "
                              '(objectives.py:595-601)')
