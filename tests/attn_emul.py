"""Torch emulation of the arithmetic of the training path's attention kernels as csrc/attention.hip states it: fp32
everywhere, the probabilities, dS and every output rounded to bf16 once, delta from the bf16 ctx.  Runs on the CPU.

  fwd_lazy    attn_fwd1_kernel: 32-key tiles, the reference maximum in raw score units, rescaled only when some row of
              the 32-query wave outgrew it by more than 8 / scale_log2e
  fwd_exact   attn_fwd_kernel / attn_fwd_long_kernel: 128-key chunks, an exact running maximum in log2 units
  bwd         attn_bwd1_kernel and the streaming pair: p rebuilt from lse, dS = p (keep dP - delta keep_prob)

`mut` names planted errors (tests/test_attention_bounds_cpu.py shows that the bounds of tests/attn_cases.py catch them):
  l_norescale, O_norescale   the row sum / the accumulators are not rescaled after the first tile (chunk)
  lse_unit                   lse built with the maximum in the wrong unit
  delta_neighbor             delta taken from the neighbouring row
  kbias9                     the key bias of the ninth tile ignored
  dropmask9                  the backward's dropout mask all-true in the ninth key tile
  no_inv_keep_dv             inv_keep missing in dv"""
import torch

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
NEG = float('-inf')


def _bf(x):
    return x.to(torch.bfloat16).float()


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def _scores(q, k, init):
    """init[i, j] + sum_d q[i, d] k[j, d], the 64 exact bf16 products added one at a time in fp32 in feature order: one
    rounding per addition, the same on every machine (a BLAS product would leave the order open)"""
    S = init.clone()
    for dd in range(q.shape[1]):
        S = S + q[:, dd:dd + 1] * k[:, dd][None, :]
    return S


def _pad(n, q, k, v, kb, keep):
    """padded tokens read the last real row; their key bias is -inf"""
    npd = ((n + 31) // 32) * 32
    idx = torch.arange(npd).clamp(max=n - 1)
    kbp = torch.cat([kb, torch.full((npd - n,), NEG)])
    kp = torch.ones(npd, npd)
    if keep is not None:
        kp[:n, :n] = keep.float()
    return npd, q[idx], k[idx], v[idx], kbp, kp


def fwd_lazy(q, k, v, kb, scale, keep=None, inv_keep=1.0, mut=()):
    n = q.shape[0]
    npd, q, k, v, kb, kp = _pad(n, q, k, v, kb, keep)
    nt = npd // 32
    c2 = _f32(scale * LOG2E)
    thr = 8.0 / c2
    S_all = _scores(q, k, kb[None, :].expand(npd, npd))
    m = torch.full((npd,), NEG)
    l = torch.zeros(npd)
    O = torch.zeros(npd, 64)
    for t in range(nt):
        tile = slice(t * 32, t * 32 + 32)
        S = S_all[:, tile]
        mx = S.max(1).values
        trig = ((mx - m) > thr).view(nt, 32).any(1).repeat_interleave(32)      # the wave-uniform branch
        m_new = torch.maximum(m, mx)
        alpha = torch.where(m == NEG, torch.ones(()), torch.exp2((m - m_new) * c2))
        alpha = torch.where(trig, alpha, torch.ones(()))
        if not ('l_norescale' in mut and t > 0):
            l = l * alpha
        if not ('O_norescale' in mut and t > 0):
            O = O * alpha[:, None]
        m = torch.where(trig, m_new, m)
        msub = torch.where(m == NEG, torch.zeros(()), -m * c2)
        p = torch.exp2(S * c2 + msub[:, None])
        l = l + p.sum(1)
        O = O + _bf(p * kp[:, tile]) @ v[tile]
    ctx = _bf(O * (inv_keep / l)[:, None])
    lse = ((m if 'lse_unit' in mut else m * c2) + torch.log2(l)) * LN2
    return ctx[:n], lse[:n]


def fwd_exact(q, k, v, kb, scale, keep=None, inv_keep=1.0, mut=(), chunk=128):
    n = q.shape[0]
    npd, q, k, v, kb, kp = _pad(n, q, k, v, kb, keep)
    c2 = _f32(scale * LOG2E)
    T_all = _scores(q, k, torch.zeros(npd, npd)) * c2 + kb[None, :]
    m = torch.full((npd,), NEG)
    l = torch.zeros(npd)
    O = torch.zeros(npd, 64)
    for c0 in range(0, npd, chunk):
        ch = slice(c0, min(c0 + chunk, npd))
        T = T_all[:, ch]
        m_new = torch.maximum(m, T.max(1).values)
        dead = m_new == NEG
        alpha = torch.where(dead, torch.ones(()), torch.exp2(m - m_new))
        p = torch.where(dead[:, None], torch.zeros(()), torch.exp2(T - m_new[:, None]))
        l = (l if ('l_norescale' in mut and c0 > 0) else l * alpha) + p.sum(1)
        if not ('O_norescale' in mut and c0 > 0):
            O = O * alpha[:, None]
        m = m_new
        O = O + _bf(p * kp[:, ch]) @ v[ch]
    ctx = _bf(O * (inv_keep / l)[:, None])
    lse = ((m / c2 if 'lse_unit' in mut else m) + torch.log2(l)) * LN2
    return ctx[:n], lse[:n]


def bwd(q, k, v, dO, ctx, lse, kb, scale, keep=None, inv_keep=1.0, mut=()):
    """ctx: the forward's bf16 output (as fp32 values).  Returns bf16-rounded dq, dk, dv and the fp32 column sums of the
    unrounded dq | dv."""
    n = q.shape[0]
    c2 = _f32(scale * LOG2E)
    keep_prob = _f32(1.0) / _f32(inv_keep)
    out_scale = _f32(scale) * _f32(inv_keep)
    delta = (ctx * dO).sum(1)
    if 'delta_neighbor' in mut:
        delta = delta.roll(1)
    S = _scores(q, k, (-lse * (1.0 / _f32(scale)))[:, None].expand(n, n))
    p = torch.exp2(S * c2 + kb[None, :])
    kp = keep.float().clone() if keep is not None else torch.ones(n, n)
    if 'dropmask9' in mut:
        kp[:, 256:288] = 1.0
    pd = p * kp
    dP = dO @ v.T
    sf = _bf(pd * dP + p * (-delta * keep_prob)[:, None])
    pf = _bf(pd)
    dV = (pf.T @ dO) * (1.0 if 'no_inv_keep_dv' in mut else _f32(inv_keep))
    dK = (sf.T @ q) * out_scale
    dQ = (sf @ k) * out_scale
    return _bf(dQ), _bf(dK), _bf(dV), torch.cat([dQ.sum(0), dV.sum(0)])


def run(case, keep=None, inv_keep=1.0, scale=64 ** -0.5, mut=(), forward=None):
    """the whole launch of a tests/attn_cases.Case the way vlmo_attn_fwd / vlmo_attn_bwd dispatch it (the launch's
    max_len picks the forward: lazy up to 288 tokens, exact above; `forward` overrides).  Returns ctx, lse, dqkv, qv
    shaped as the kernels write them."""
    d, H, M = case.d, case.heads, case.M
    X = case.qkv.float().cpu()
    dO_all = case.dctx.float().cpu()
    km = case.keymask.cpu()
    fwd = forward or (fwd_lazy if case.max_len <= 288 else fwd_exact)
    npd = ((case.max_len + 31) // 32) * 32
    ctx = torch.full((M, d), float('nan'))
    dqkv = torch.full((M, 3 * d), float('nan'))
    lse = torch.full((len(case.lens) * H, npd), float('nan'))
    qv = torch.zeros(len(case.lens), 2 * d)
    for s, rows in enumerate(case.rows):
        rows = rows.cpu()
        n = len(rows)
        kb = torch.where(km[rows] != 0, torch.zeros(()), torch.full((), NEG))
        if 'kbias9' in mut:
            kb[256:288] = 0.0
        for hd in range(H):
            c = slice(hd * 64, hd * 64 + 64)
            q, k, v, dO = X[rows][:, c], X[rows][:, d:2 * d][:, c], X[rows][:, 2 * d:][:, c], dO_all[rows][:, c]
            kp = keep[s, hd, :n, :n] if keep is not None else None
            o, l = fwd(q, k, v, kb, scale, kp, inv_keep, mut)
            dq, dk, dv, cs = bwd(q, k, v, dO, o, l, kb, scale, kp, inv_keep, mut)
            col = torch.arange(hd * 64, hd * 64 + 64)
            ctx[rows[:, None], col[None, :]] = o
            for third, x in enumerate((dq, dk, dv)):
                dqkv[rows[:, None], third * d + col[None, :]] = x
            lse[s * H + hd, :n] = l
            qv[s, c] = cs[:64]
            qv[s, d + hd * 64:d + hd * 64 + 64] = cs[64:]
    return dict(ctx=ctx, lse=lse, dqkv=dqkv, qv=qv)
