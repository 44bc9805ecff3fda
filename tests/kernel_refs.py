"""Helpers shared by the per-kernel GPU tests (tests/test_kernels_gpu.py, tests/test_launch_regimes_gpu.py and the files
that build on them): gaussian operands, the element-wise comparison, the packed attention case, its fp32 torch reference
and the host replica of the attention kernels' dropout mask.  A plain module: importing it needs no device."""
import numpy as np
import torch

from tests.dropmask import hash32 as _hash32

DEV = 'cuda'


def _rand(*shape, scale=1.0, seed=0, dtype=torch.bfloat16):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def _close(got, ref, rtol, atol, what=''):
    got, ref = got.float(), ref.float()
    err = (got - ref).abs()
    lim = atol + rtol * ref.abs()
    bad = err > lim
    if bad.any():
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(
            f'{what}: {int(bad.sum())}/{bad.numel()} mismatches, max err {err.max().item():.4g} '
            f'first at {idx}: got {got[tuple(idx)].item():.6g} ref {ref[tuple(idx)].item():.6g}')


def _attn_case(B, lenA, lenB, heads, seed=0, mask_frac=0.3):
    """packed rows: all A segments, then all B segments."""
    d = heads * 64
    M = B * (lenA + lenB)
    qkv = _rand(M, 3 * d, seed=seed, scale=1.0)
    seg = torch.tensor([[b * lenA, lenA, B * lenA + b * lenB, lenB] for b in range(B)], dtype=torch.int32)
    keymask = torch.ones(M, dtype=torch.int32)
    g = torch.Generator().manual_seed(seed + 1)
    for b in range(B):
        if b % 2 == 1 and lenA > 4:
            p0 = int(torch.randint(2, lenA, (1,), generator=g))
            keymask[b * lenA + p0:(b + 1) * lenA] = 0
    return qkv, seg.to(DEV), keymask.to(DEV), M, d


def _attn_keep_mask(seed, nseq, heads, N, thresh):
    """[nseq, heads, N(q), N(key)] bool: the keep mask of the attention kernels' counter-based dropout
    (csrc/attention.hip att_key / att_mix): top 16 bits of mix((q * 512 + key) * G + key(seed, bh)) >= thresh."""
    m = np.uint64(0xFFFFFFFF)
    bh = (np.arange(nseq, dtype=np.uint64)[:, None] * np.uint64(heads) + np.arange(heads, dtype=np.uint64)[None, :])
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    akey = (_hash32((lo ^ ((bh * np.uint64(0x9E3779B9)) & m)) & m) + hi) & m
    q = np.arange(N, dtype=np.uint64)[None, None, :, None]
    key = np.arange(N, dtype=np.uint64)[None, None, None, :]
    x = ((((q * np.uint64(512) + key) & m) * np.uint64(0x9E3779B1)) + akey[:, :, None, None]) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x7feb352d)) & m
    return torch.from_numpy((x >> np.uint64(16)) >= np.uint64(thresh))


def _attn_ref(qkv, seg, keymask, heads, d, dctx=None, keep=None, inv_keep=1.0):
    """fp32 torch reference per sequence (vlmo.py:79-95); returns ctx (+ dqkv).  keep: optional dropout keep
    mask [nseq, heads, N, N] applied to the probabilities (vlmo.py:93)."""
    q = qkv.float().clone().requires_grad_(dctx is not None)
    ctx = torch.zeros(q.shape[0], d, device=q.device)
    outs = []
    for si, s in enumerate(seg.tolist()):
        rows = torch.cat([torch.arange(s[0], s[0] + s[1]), torch.arange(s[2], s[2] + s[3])]).to(q.device)
        x = q[rows]
        N = x.shape[0]
        qq, kk, vv = [x[:, i * d:(i + 1) * d].reshape(N, heads, 64).transpose(0, 1) for i in range(3)]
        att = (qq @ kk.transpose(-2, -1)) * 64 ** -0.5
        att = att.masked_fill(~keymask[rows].bool()[None, None, :], float('-inf')).softmax(-1)
        if keep is not None:
            att = att * keep[si, :, :N, :N].to(att.device) * inv_keep
        o = (att @ vv).transpose(0, 1).reshape(N, d)
        outs.append((rows, o))
    ctx = torch.zeros(q.shape[0], d, device=q.device)
    for rows, o in outs:
        ctx = ctx.index_add(0, rows, o)
    if dctx is None:
        return ctx.detach()
    ctx.backward(dctx.float())
    return ctx.detach(), q.grad


def _attn_lse_close(lse, qkv, seg, keymask, heads, d, what=''):
    """the forward's log-sum-exp [nseq * heads, >= N] against fp64 torch per sequence and head, at the tolerance
    a + b |lse| of tests/attn_cases.py (four times the error of an fp32 emulation of the kernels' formula)"""
    from tests.attn_cases import lse_tol
    x = qkv.double()
    for si, s in enumerate(seg.tolist()):
        rows = torch.cat([torch.arange(s[0], s[0] + s[1]), torch.arange(s[2], s[2] + s[3])]).to(x.device)
        N = len(rows)
        qq, kk = [x[rows][:, i * d:(i + 1) * d].reshape(N, heads, 64).transpose(0, 1) for i in range(2)]
        att = (qq @ kk.transpose(-2, -1)) * 64 ** -0.5
        want = att.masked_fill(~keymask[rows].bool()[None, None, :], float('-inf')).logsumexp(-1)
        have = lse[si * heads:(si + 1) * heads, :N].double()
        bad = ~((have - want).abs() <= lse_tol(want))             # a NaN left in lse is bad
        if bad.any():
            idx = bad.nonzero()[0].tolist()
            raise AssertionError(f'attn lse {what}: sequence {si}, {int(bad.sum())}/{bad.numel()} mismatches, first at '
                                 f'{idx}: got {have[tuple(idx)].item():.9g} ref {want[tuple(idx)].item():.9g}')
