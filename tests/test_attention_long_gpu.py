"""Attention over sequences of up to 1024 tokens (img_size 384 / 480: 577 / 901 image tokens, 593 - 965 in the fused
layers): the streaming kernels of csrc/attention.hip, forward for launches of 513 - 1024 tokens, backward (dK/dV and
dQ kernels) for 289 - 1024, against fp32 torch with the tolerances of tests/test_kernels_gpu.py."""
import pytest
import torch

from exploremultimodal_amd import hip
from tests import attn_counter
from tests.kernel_refs import _attn_case, _attn_lse_close, _attn_ref, _close, _rand

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SCALE = 64 ** -0.5


def _rows(sg):
    return torch.cat([torch.arange(sg[0], sg[0] + sg[1]), torch.arange(sg[2], sg[2] + sg[3])]).to(DEV)


def _lens(seg):
    return [s[1] + s[3] for s in seg.tolist()]


def _npad(n):
    return ((n + 31) // 32) * 32


def _fwd_bwd(qkv, seg, keymask, heads, d, max_len, dctx, drop=None, seed=0):
    nseq = seg.shape[0]
    kw = dict(drop=drop, seed=seed) if drop else {}
    M = qkv.shape[0]
    ctx = torch.full((M, d), float('nan'), device=DEV, dtype=torch.bfloat16)
    lse = torch.full((nseq * heads, _npad(max_len)), float('nan'), device=DEV)
    hip.attn_fwd(qkv, seg, nseq, keymask, ctx, lse, heads, d, max_len, SCALE, **kw)
    dqkv = torch.full((M, 3 * d), float('nan'), device=DEV, dtype=torch.bfloat16)
    qv = torch.full((nseq, 2 * d), float('nan'), device=DEV)
    hip.attn_bwd(qkv, ctx, dctx, lse, seg, nseq, keymask, dqkv, heads, d, max_len, SCALE, qv_colsum=qv, **kw)
    torch.cuda.synchronize()
    return ctx, lse, dqkv, qv


def _check(qkv, seg, keymask, heads, d, ctx, dqkv, qv, dctx, keep=None, inv_keep=1.0, what='', *, lse):
    ref_ctx, ref_dqkv = _attn_ref(qkv, seg, keymask, heads, d, dctx, keep=keep, inv_keep=inv_keep)
    _close(ctx, ref_ctx, 1 / 64, 1e-2, f'attn ctx {what}')
    _attn_lse_close(lse, qkv, seg, keymask, heads, d, what)
    scale = ref_dqkv.abs().max().item()
    _close(dqkv, ref_dqkv, 1 / 32, 2e-2 * scale, f'attn dqkv {what}')
    for si, sg in enumerate(seg.tolist()):
        rows = _rows(sg)
        want = torch.cat([ref_dqkv[rows, :d].sum(0), ref_dqkv[rows, 2 * d:].sum(0)])
        _close(qv[si], want, 1 / 32, 2e-2 * scale * max(1.0, len(rows) ** 0.5), f'attn qv column sums {what} seq {si}')


@pytest.mark.parametrize('B,lenA,lenB,heads', [(2, 40, 577, 2), (1, 0, 577, 1), (1, 64, 901, 2), (1, 0, 1024, 1),
                                               (2, 16, 497, 2), (1, 0, 289, 1)])
def test_long_attention_fwd_bwd(B, lenA, lenB, heads):
    qkv, seg, keymask, M, d = _attn_case(B, lenA, lenB, heads, seed=B + lenA + lenB)
    N = lenA + lenB
    dctx = _rand(M, d, seed=77)
    ctx, lse, dqkv, qv = _fwd_bwd(qkv, seg, keymask, heads, d, N, dctx)
    _check(qkv, seg, keymask, heads, d, ctx, dqkv, qv, dctx, what=f'N={N}', lse=lse)


def _mixed_case(heads=2, seed=21):
    lens = [1024, 700, 577, 513, 300, 40]
    d = heads * 64
    starts = [sum(lens[:i]) for i in range(len(lens))]
    M = sum(lens)
    qkv = _rand(M, 3 * d, seed=seed, scale=1.0)
    seg = [[s, n, 0, 0] for s, n in zip(starts, lens)]
    seg[1] = [starts[1], 60, starts[1] + 60, 640]            # a packed two-range sequence like a fused text + image one
    seg = torch.tensor(seg, dtype=torch.int32).to(DEV)
    keymask = torch.ones(M, dtype=torch.int32)
    keymask[starts[1] + 30:starts[1] + 60] = 0               # padded text keys of the packed sequence
    keymask[starts[3] + 500:starts[3] + 513] = 0             # the fringe keys of the 513-token sequence
    keymask[starts[5] + 25:starts[5] + 40] = 0
    return qkv, seg, keymask.to(DEV), M, d, heads, lens


@pytest.mark.parametrize('dropout', [False, True])
def test_long_attention_mixed_lengths_in_one_launch(dropout):
    qkv, seg, keymask, M, d, heads, lens = _mixed_case()
    drop = hip.drop_params(0.1, True) if dropout else None
    seed = 0x5EED5EED1
    dctx = _rand(M, d, seed=81)
    ctx, lse, dqkv, qv = _fwd_bwd(qkv, seg, keymask, heads, d, max(lens), dctx, drop=drop, seed=seed)
    keep = attn_counter.keep_mask(seed, lens, heads, drop[0]) if dropout else None
    _check(qkv, seg, keymask, heads, d, ctx, dqkv, qv, dctx, keep=keep, inv_keep=drop[1] if dropout else 1.0,
           what='(mixed)', lse=lse)


@pytest.mark.parametrize('B,lenA,lenB,heads', [(2, 40, 577, 2), (1, 64, 901, 1), (1, 0, 289, 1), (2, 16, 497, 1)])
def test_long_attention_dropout_forward_and_backward_use_the_same_mask(B, lenA, lenB, heads):
    """the forward (resident kernels up to 512 tokens, streaming above) and the streaming backward against the fp32
    reference under the host replica of the per-sequence counter rule"""
    qkv, seg, keymask, M, d = _attn_case(B, lenA, lenB, heads, seed=17 + lenB)
    N = lenA + lenB
    drop = hip.drop_params(0.1, True)
    seed = 0x1234567ABCDEF01
    keep = attn_counter.keep_mask(seed, _lens(seg), heads, drop[0])
    assert abs(keep.float().mean().item() - 0.9) < 0.01
    dctx = _rand(M, d, seed=78)
    ctx, lse, dqkv, qv = _fwd_bwd(qkv, seg, keymask, heads, d, N, dctx, drop=drop, seed=seed)
    _check(qkv, seg, keymask, heads, d, ctx, dqkv, qv, dctx, keep=keep, inv_keep=drop[1], what=f'(dropout, N={N})', lse=lse)


def test_split_backward_of_a_shared_384px_launch_regenerates_the_forward_mask():
    """Below the fusion layer at 384 px one forward launch holds the B image sequences (577 tokens) and then the B text
    sequences (40): max_len 577.  Backward as two launches -- the image sequences (max_len 577, mask_seq0 0, the
    streaming kernels) and the text sequences (max_len 40, mask_seq0 B, the resident kernels) -- gives the dqkv of one
    backward launch over all of them: the text sequences' dropout counter follows their own length, not the launch's."""
    B, P, T, heads = 2, 577, 40, 2
    d = heads * 64
    M = B * (P + T)
    qkv = _rand(M, 3 * d, seed=31, scale=1.0)
    seg = torch.tensor([[B * T + b * P, P, 0, 0] for b in range(B)] + [[b * T, T, 0, 0] for b in range(B)],
                       dtype=torch.int32).to(DEV)
    keymask = torch.ones(M, dtype=torch.int32)
    keymask[T + 20:2 * T] = 0
    keymask = keymask.to(DEV)
    drop = hip.drop_params(0.1, True)
    seed = 0xFEEDBEEF42
    kw = dict(drop=drop, seed=seed)
    dctx = _rand(M, d, seed=82)
    ctx, lse, dqkv1, qv1 = _fwd_bwd(qkv, seg, keymask, heads, d, P, dctx, drop=drop, seed=seed)
    dqkv2 = torch.full_like(dqkv1, float('nan'))
    qv2 = torch.full_like(qv1, float('nan'))
    hip.attn_bwd(qkv, ctx, dctx, lse[:B * heads], seg[:B], B, keymask, dqkv2, heads, d, P, SCALE,
                 qv_colsum=qv2[:B], **kw)
    hip.attn_bwd(qkv, ctx, dctx, lse[B * heads:], seg[B:], B, keymask, dqkv2, heads, d, T, SCALE,
                 qv_colsum=qv2[B:], mask_seq0=B, **kw)
    torch.cuda.synchronize()
    keep = attn_counter.keep_mask(seed, _lens(seg), heads, drop[0])
    _check(qkv, seg, keymask, heads, d, ctx, dqkv1, qv1, dctx, keep=keep, inv_keep=drop[1], what='(one launch)', lse=lse)
    _check(qkv, seg, keymask, heads, d, ctx, dqkv2, qv2, dctx, keep=keep, inv_keep=drop[1], what='(split)', lse=lse)
    # the image rows are the same kernels on the same operands: bit-identical; the text rows come from another kernel
    img = torch.arange(B * T, M, device=DEV)
    assert torch.equal(dqkv1[img], dqkv2[img])
    _close(dqkv2, dqkv1, 1 / 32, 2e-2 * dqkv1.float().abs().max().item(), 'split vs one launch')


def test_long_attention_backward_is_bitwise_reproducible():
    qkv, seg, keymask, M, d, heads, lens = _mixed_case(seed=23)
    drop = hip.drop_params(0.1, True)
    dctx = _rand(M, d, seed=83)
    ctx, lse, dqkv1, qv1 = _fwd_bwd(qkv, seg, keymask, heads, d, max(lens), dctx, drop=drop, seed=99)
    for _ in range(2):
        dqkv2 = torch.full_like(dqkv1, float('nan'))
        qv2 = torch.full_like(qv1, float('nan'))
        hip.attn_bwd(qkv, ctx, dctx, lse, seg, len(lens), keymask, dqkv2, heads, d, max(lens), SCALE,
                     drop=drop, seed=99, qv_colsum=qv2)
        torch.cuda.synchronize()
        assert torch.equal(dqkv1, dqkv2)
        assert torch.equal(qv1, qv2)


def test_sequences_above_1024_tokens_are_refused():
    heads, N = 1, 1025
    qkv, seg, keymask, M, d = _attn_case(1, 0, N, heads)
    ctx = torch.zeros(M, d, device=DEV, dtype=torch.bfloat16)
    lse = torch.zeros(heads, _npad(N), device=DEV)
    with pytest.raises(RuntimeError, match='exceeds'):
        hip.attn_fwd(qkv, seg, 1, keymask, ctx, lse, heads, d, N, SCALE)
    dqkv = torch.zeros(M, 3 * d, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match='exceeds'):
        hip.attn_bwd(qkv, ctx, ctx, lse, seg, 1, keymask, dqkv, heads, d, N, SCALE)
    torch.cuda.synchronize()
