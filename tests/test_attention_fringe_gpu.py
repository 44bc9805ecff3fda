"""The single-pass attention backward at 257 .. 288 tokens (csrc/attention.hip, attn_bwd1_kernel<true>): eight waves
own the eight full tiles, the ninth (fringe) tile of 1 .. 32 tokens is covered by two more steps and its rows are
combined through LDS.  dq / dk / dv and the per-sequence column sums of dq | dv against an fp32 torch reference per
sequence with the replicated dropout mask (tests/attn_counter.py), with the bounds tests/test_kernels_gpu.py uses for
this path: |err| <= 2e-2 max|ref| + |ref| / 32 per element, the column sums with the sqrt(rows) factor.  Every case
pre-fills dqkv with NaN (every row of every real token must be written, the k and v thirds of masked keys too) and
runs the backward twice: the two dqkv must be bitwise equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from exploremultimodal_amd import hip  # noqa: E402
from tests import attn_counter  # noqa: E402

DEV = 'cuda'
SCALE = 64 ** -0.5
SEED = 0xF00D5EED77


def _rand(*shape, seed=0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV).to(torch.bfloat16)


def _rows(sg):
    return torch.cat([torch.arange(sg[0], sg[0] + sg[1]), torch.arange(sg[2], sg[2] + sg[3])]).to(DEV)


def _attn_ref(qkv, seg, keymask, heads, d, dctx, keep, inv_keep):
    """fp32 torch reference per sequence (softmax(q k^T / 8 + keymask) ; dropout ; @ v): dqkv"""
    q = qkv.float().clone().requires_grad_(True)
    ctx = torch.zeros(q.shape[0], d, device=q.device)
    for si, s in enumerate(seg.tolist()):
        rows = _rows(s)
        x = q[rows]
        N = x.shape[0]
        qq, kk, vv = [x[:, i * d:(i + 1) * d].reshape(N, heads, 64).transpose(0, 1) for i in range(3)]
        att = (qq @ kk.transpose(-2, -1)) * SCALE
        att = att.masked_fill(~keymask[rows].bool()[None, None, :], float('-inf')).softmax(-1)
        if keep is not None:
            att = att * keep[si, :, :N, :N].to(att.device) * inv_keep
        ctx = ctx.index_add(0, rows, (att @ vv).transpose(0, 1).reshape(N, d))
    ctx.backward(dctx.float())
    return q.grad


def _close(got, ref, atol, what):
    got, ref = got.float(), ref.float()
    err = (got - ref).abs()
    bad = ~(err <= atol + ref.abs() / 32)           # a NaN left in `got` is bad
    if bad.any():
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {err[~err.isnan()].max().item():.4g}, '
                             f'first at {idx}: got {got[tuple(idx)].item():.6g} ref {ref[tuple(idx)].item():.6g}')


def _check(seg, keymask, heads, dropout, with_qv, seed=SEED):
    """forward + backward of one launch over `seg` ([nseq][4] row ranges), checked against the reference; returns
    (qkv, ctx, dctx, lse, dqkv) for the tests that go on from there"""
    d = heads * 64
    seg_t = torch.tensor(seg, dtype=torch.int32).to(DEV)
    lens = [s[1] + s[3] for s in seg]
    nseq, N = len(seg), max(lens)
    M = max(max(s[0] + s[1], s[2] + s[3]) for s in seg)
    assert 256 < N <= 288
    qkv = _rand(M, 3 * d, seed=N + nseq)
    dctx = _rand(M, d, seed=N + nseq + 1)
    keymask = keymask.to(DEV)
    drop = hip.drop_params(0.1, True) if dropout else None
    kw = dict(drop=drop, seed=seed) if drop else {}
    ctx = torch.zeros(M, d, device=DEV, dtype=torch.bfloat16)
    lse = torch.zeros(nseq * heads, 288, device=DEV)
    hip.attn_fwd(qkv, seg_t, nseq, keymask, ctx, lse, heads, d, N, SCALE, **kw)
    keep = attn_counter.keep_mask(seed, lens, heads, drop[0], npad=N) if drop else None
    ref = _attn_ref(qkv, seg_t, keymask, heads, d, dctx, keep, drop[1] if drop else 1.0)
    out = []
    for _ in range(2):
        dqkv = torch.full((M, 3 * d), float('nan'), device=DEV, dtype=torch.bfloat16)
        qv = torch.full((nseq, 2 * d), float('nan'), device=DEV) if with_qv else None
        hip.attn_bwd(qkv, ctx, dctx, lse, seg_t, nseq, keymask, dqkv, heads, d, N, SCALE, qv_colsum=qv, **kw)
        out.append(dqkv)
    scale = ref.abs().max().item()
    used = torch.cat([_rows(s) for s in seg])
    _close(out[0][used], ref[used], 2e-2 * scale, 'dqkv')
    assert torch.equal(out[0][used].view(torch.int16), out[1][used].view(torch.int16)), 'dqkv differs between two runs'
    if with_qv:
        for si, sg in enumerate(seg):
            rows = _rows(sg)
            want = torch.cat([ref[rows, :d].sum(0), ref[rows, 2 * d:].sum(0)])
            _close(qv[si], want, 2e-2 * scale * len(rows) ** 0.5, f'qv column sums, sequence {si}')
    return qkv, ctx, dctx, lse, out[0], seg_t, keymask


def _plain(lens):
    seg, r = [], 0
    for n in lens:
        seg.append([r, n, 0, 0])
        r += n
    return seg, r


@pytest.mark.parametrize('with_qv', [True, False])
@pytest.mark.parametrize('dropout', [False, True])
@pytest.mark.parametrize('N,heads', [(257, 1), (261, 2), (272, 1), (288, 2)])
def test_one_length_alone_in_a_launch(N, heads, dropout, with_qv):
    """fringes of 1, 5 (the workload's), 16 and 32 tokens"""
    seg, M = _plain([N])
    _check(seg, torch.ones(M, dtype=torch.int32), heads, dropout, with_qv)


@pytest.mark.parametrize('dropout', [False, True])
def test_packed_text_and_image_ranges(dropout):
    """64 text + 197 image rows per sequence, all text rows first as the fused layers have them; part of the text range
    of the second sequence is masked"""
    B, T, P = 2, 64, 197
    seg = [[b * T, T, B * T + b * P, P] for b in range(B)]
    keymask = torch.ones(B * (T + P), dtype=torch.int32)
    keymask[T + 23:2 * T] = 0
    _check(seg, keymask, 2, dropout, True)


@pytest.mark.parametrize('with_qv', [True, False])
@pytest.mark.parametrize('dropout', [False, True])
def test_mixed_launch(dropout, with_qv):
    """fringe sequences, a full eight-tile one and sequences of fewer tiles share one launch"""
    seg, M = _plain([261, 64, 256, 200, 288])
    keymask = torch.ones(M, dtype=torch.int32)
    keymask[261 + 50:261 + 64] = 0
    _check(seg, keymask, 2, dropout, with_qv)


@pytest.mark.parametrize('dropout', [False, True])
def test_key_masks_over_fringe_core_tile_and_text_range(dropout):
    seg = [[0, 270, 0, 0], [270, 261, 0, 0], [531, 64, 595, 197]]
    keymask = torch.ones(595 + 197, dtype=torch.int32)
    keymask[256:270] = 0                    # the whole fringe of sequence 0
    keymask[270 + 96:270 + 128] = 0         # a whole core tile of sequence 1
    keymask[531 + 1:531 + 64] = 0           # all keys of the text range of sequence 2 but one
    _check(seg, keymask, 1, dropout, True)


def test_suffix_launch_regenerates_the_mask_of_the_whole_launch():
    """mask_seq0 > 0: a launch over the last sequences equals the matching rows of the launch over all of them"""
    heads = 2
    d = heads * 64
    seg, M = _plain([261, 280, 261, 257])
    qkv, ctx, dctx, lse, dqkv, seg_t, keymask = _check(seg, torch.ones(M, dtype=torch.int32), heads, True, True)
    drop = hip.drop_params(0.1, True)
    s0 = 2
    part = torch.full((M, 3 * d), float('nan'), device=DEV, dtype=torch.bfloat16)
    hip.attn_bwd(qkv, ctx, dctx, lse[s0 * heads:], seg_t[s0:].contiguous(), len(seg) - s0, keymask, part, heads, d, 261,
                 SCALE, drop=drop, seed=SEED, mask_seq0=s0)
    r0 = seg[s0][0]
    assert torch.equal(part[r0:].view(torch.int16), dqkv[r0:].view(torch.int16))
    assert part[:r0].isnan().all()
