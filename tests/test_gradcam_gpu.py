"""vlmo_attn_gradcam (the gradient-weighted attention-map kernel) against attnmap.attention_gradcam_reference in fp64 on
the same bf16 values, in the style of tests/test_attnmap_gpu.py.

Every launch writes into a NaN-filled buffer between two sentinel guard regions; every qkv and dctx row that belongs to
no sequence of the launch is NaN, so a read outside the segments or a write outside the output shows.

The bound is derived, not tuned (u = 2^-24, gamma = 64 u / (1 - 64 u)).
  * P: products of bf16 values are exact in fp32, so only the 64-term fp32 sum moves a score, by at most gamma * scale *
    sum |q_i| |k_i|; a score error e moves a probability by a factor exp(e) on top and, through the row sum, on the bottom:
    the kernel's P is P64 (1 + delta), |delta| <= rel = 2 gamma scale max_ij (|q| @ |k|^T)_ij + 8 u (that file's factor).
  * G = dctx . v^T is the same kind of sum: |G - G64| <= eG = gamma (|dctx| @ |v|^T), elementwise per head.
  * 'cam' and 'attn_grad': out = P * f(G) with f = max(., 0) or the identity, both 1-Lipschitz, so |f(G) - f(G64)| <= eG and
        |out - want| <= |delta| P64 |f(G64)| + (1 + rel) P64 eG + (roundings of the product and of 1 / heads)
                     <= rel |want| + (1 + rel) P64 eG + 8 u |want| + 1e-30.
  * 'grad': |G - G64| <= eG + 8 u |G64| + 1e-30.
  * head_mean: the mean over heads of the per-head bounds, plus heads * u * mean_h |want| for the fp32 additions.
Where the definition says zero, the output must be exactly zero, for every kind."""
import pytest
import torch

from exploremultimodal_amd import attnmap, hip

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
GAMMA = 64 * U / (1 - 64 * U)
SCALE = 0.125
GUARD, SENT = 4099, 12345.0
NSEQ = 3
LENGTHS = [1, 33, 64, 261, 512, 513, 1024]
KINDS = ('cam', 'attn_grad', 'grad')


def _layout(L, heads, two_range, seed):
    """qkv [M, 3d] and dctx [M, d] bf16 with NaN outside the sequences, seg [3, 4], rows-of-token lists.  Sequence 1 is
    shorter than L; in the two-range form the second range lies BEFORE the first in memory."""
    lens = [L, max(1, L - 3), L]
    seg, tok_rows, row = [], [], 0
    for n in lens:
        len_a = n - n // 3 if two_range else n
        len_b = n - len_a
        row += 2
        row_b = row
        row += len_b + 3
        row_a = row
        row += len_a + 1
        seg.append([row_a, len_a, row_b if len_b else 0, len_b])
        tok_rows.append(torch.cat([torch.arange(row_a, row_a + len_a), torch.arange(row_b, row_b + len_b)]))
    M = row + 5
    g = torch.Generator().manual_seed(seed)
    qkv = torch.full((M, 3 * 64 * heads), float('nan'))
    dctx = torch.full((M, 64 * heads), float('nan'))
    used = torch.cat(tok_rows)
    qkv[used] = torch.randn(used.numel(), 3 * 64 * heads, generator=g)
    dctx[used] = torch.randn(used.numel(), 64 * heads, generator=g)
    seg = torch.tensor(seg, dtype=torch.int32, device=DEV)
    return qkv.bfloat16().to(DEV), dctx.bfloat16().to(DEV), seg, tok_rows, M, g


def _masks(L, tok_rows, M, g):
    """none, a padded tail in sequence 0, scattered zeros, sequence 2 fully masked."""
    tail = torch.ones(M, dtype=torch.int32)
    tail[tok_rows[0][L - L // 3:]] = 0
    scat = (torch.rand(M, generator=g) >= 0.3).to(torch.int32)
    full = torch.ones(M, dtype=torch.int32)
    full[tok_rows[2]] = 0
    return {'none': None, 'tail': tail.to(DEV), 'scattered': scat.to(DEV), 'seq2_masked': full.to(DEV)}


def _windows(L):
    q0 = min(5, L - 1)
    return [(0, L), (0, 1), (q0, min(37, L - q0)), (L - 1, 1)]


def _launch(qkv, dctx, seg, nseq, km, heads, L, q0, nq, kind, head_mean, scale=SCALE):
    """One kernel call into a guarded, NaN-filled buffer -> the output view."""
    n = nseq * (1 if head_mean else heads) * nq * L
    buf = torch.full((GUARD + n + GUARD,), SENT, device=DEV)
    buf[GUARD:GUARD + n] = float('nan')
    out = buf[GUARD:GUARD + n]
    hip.attn_gradcam(qkv, dctx, seg, nseq, km, out, heads, 64 * heads, L, q0, nq, kind, head_mean, scale)
    assert (buf[:GUARD] == SENT).all() and (buf[GUARD + n:] == SENT).all(), 'wrote outside the output'
    return out.view(nseq, 1 if head_mean else heads, nq, L)


def _rel_factor(qkv, heads, tok_rows):
    d = 64 * heads
    worst = 0.0
    for rows in tok_rows:
        x = qkv[rows.to(DEV)].float().abs()
        for h in range(heads):
            worst = max(worst, (x[:, 64 * h:64 * h + 64] @ x[:, d + 64 * h:d + 64 * h + 64].T).max().item())
    return 2 * GAMMA * SCALE * worst + 8 * U


def _wants_and_bounds(qkv, dctx, seg, heads, L, km, rel):
    """Per head, full window, fp64: {kind: (want, bound)} from the restatement alone."""
    ref = dict(seg=seg, num_seq=NSEQ, seq_len=L, heads=heads, keymask=km, scale=SCALE, dtype=torch.float64)
    P = attnmap.attention_probs_reference(qkv, **{k: v for k, v in ref.items()})
    G = attnmap.attention_gradcam_reference(qkv, dctx, kind='grad', **ref)
    eG = GAMMA * attnmap.attention_gradcam_reference(qkv.float().abs(), dctx.float().abs(), kind='grad', **ref)
    assert not torch.isnan(P).any() and not torch.isnan(G).any() and not torch.isnan(eG).any()
    out = {}
    for kind in KINDS:
        want = attnmap.attention_gradcam_reference(qkv, dctx, kind=kind, **ref)
        if kind == 'grad':
            bound = eG + 8 * U * want.abs() + 1e-30
        else:
            bound = rel * want.abs() + (1 + rel) * P * eG + 8 * U * want.abs() + 1e-30
        out[kind] = (want, bound)
    return out, P


@pytest.mark.parametrize('heads', [2, 3])
@pytest.mark.parametrize('L', LENGTHS)
def test_gradcam_matches_fp64_reference(L, heads):
    for two_range in (False, True):
        qkv, dctx, seg, tok_rows, M, g = _layout(L, heads, two_range, seed=1000 * heads + L)
        rel = _rel_factor(qkv, heads, tok_rows)
        assert rel < 5e-4                                       # the data-dependent factor stays small
        for mname, km in _masks(L, tok_rows, M, g).items():
            refs, P = _wants_and_bounds(qkv, dctx, seg, heads, L, km, rel)
            for kind in KINDS:
                want_h, bound_h = refs[kind]
                want_m = want_h.mean(dim=1, keepdim=True)
                bound_m = bound_h.mean(dim=1, keepdim=True) + heads * U * want_h.abs().mean(dim=1, keepdim=True)
                worst = 0.0
                for q0, nq in (_windows(L) if kind == 'cam' else [(0, L)]):
                    for head_mean in (False, True):
                        want = (want_m if head_mean else want_h)[:, :, q0:q0 + nq]
                        bound = (bound_m if head_mean else bound_h)[:, :, q0:q0 + nq]
                        got = _launch(qkv, dctx, seg, NSEQ, km, heads, L, q0, nq, kind, head_mean)
                        assert not torch.isnan(got).any(), (two_range, mname, kind, q0, nq, head_mean)
                        err = (got.double() - want).abs()
                        ratio = (err / bound).max().item()
                        worst = max(worst, ratio)
                        assert ratio <= 1.0, (two_range, mname, kind, q0, nq, head_mean, ratio)
                        # exact zeros wherever the definition says zero (P is zero there, for every head)
                        dead = (P.sum(dim=1, keepdim=True) if head_mean else P)[:, :, q0:q0 + nq] == 0
                        assert (got[dead] == 0).all(), (two_range, mname, kind, q0, nq, head_mean)
                print(f'L={L} H={heads} two_range={two_range} mask={mname} kind={kind}: worst error / bound {worst:.3f} '
                      f'(rel {rel:.2e})')
                # zero rules, spelled out on the full per-head output
                full = _launch(qkv, dctx, seg, NSEQ, km, heads, L, 0, L, kind, False)
                n1 = tok_rows[1].numel()
                assert (full[1, :, n1:, :] == 0).all() and (full[1, :, :, n1:] == 0).all()
                if km is not None:
                    for s in range(NSEQ):
                        masked = km[tok_rows[s].to(DEV)] == 0
                        assert (full[s][:, :, :masked.numel()][:, :, masked] == 0).all()
                        if bool(masked.all()):
                            assert (full[s] == 0).all()
                assert torch.equal(full, _launch(qkv, dctx, seg, NSEQ, km, heads, L, 0, L, kind, False))
                a = _launch(qkv, dctx, seg, NSEQ, km, heads, L, 0, L, kind, True)
                b = _launch(qkv, dctx, seg, NSEQ, km, heads, L, 0, L, kind, True)
                assert torch.equal(a, b), 'head mean is not bitwise reproducible'


def test_lengths_in_seg_are_clamped_to_seq_len():
    """Whatever seg holds, nothing outside the output is written: lengths beyond seq_len and negative ones are clamped."""
    heads, L = 2, 40
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(300, 3 * 64 * heads, generator=g).bfloat16().to(DEV)
    dctx = torch.randn(300, 64 * heads, generator=g).bfloat16().to(DEV)
    seg = torch.tensor([[10, 90, 0, 0], [100, 30, 150, 70], [200, -4, 220, 25]], dtype=torch.int32, device=DEV)
    for head_mean in (False, True):
        got = _launch(qkv, dctx, seg, 3, None, heads, L, 0, L, 'grad', head_mean)
        ref = attnmap.attention_gradcam_reference(qkv, dctx, seg, 3, L, heads, scale=SCALE, head_mean=head_mean, kind='grad',
                                                  dtype=torch.float64)
        eG = GAMMA * attnmap.attention_gradcam_reference(qkv.float().abs(), dctx.float().abs(), seg, 3, L, heads, scale=SCALE,
                                                         head_mean=head_mean, kind='grad', dtype=torch.float64)
        assert not torch.isnan(got).any()
        assert ((got.double() - ref).abs() <= eG + (8 + heads) * U * ref.abs() + 1e-30).all()
        assert (got[2, :, 25:] == 0).all() and (got[2, :, :, 25:] == 0).all()


def test_refused_arguments_return_an_error_and_write_nothing():
    heads, L = 2, 33
    qkv, dctx, seg, tok_rows, M, g = _layout(L, heads, False, seed=9)
    good = dict(nseq=NSEQ, heads=heads, L=L, q0=0, nq=L, d=64 * heads, kind=0)
    _launch(qkv, dctx, seg, NSEQ, None, heads, L, 0, L, 'cam', False)
    lib = hip.lib()
    stream = torch.cuda.current_stream().cuda_stream
    for bad in (dict(d=64 * heads + 64), dict(d=32 * heads), dict(L=0), dict(L=1025), dict(q0=-1), dict(nq=0),
                dict(q0=1), dict(q0=L, nq=1), dict(nseq=0), dict(nseq=-1), dict(kind=3), dict(kind=-1)):
        a = dict(good)
        a.update(bad)
        buf = torch.full((200000,), float('nan'), device=DEV)
        with pytest.raises(RuntimeError, match='vlmo_attn_gradcam'):
            hip.attn_gradcam(qkv, dctx, seg, a['nseq'], None, buf, a['heads'], a['d'], a['L'], a['q0'], a['nq'], a['kind'],
                             False, SCALE)
        torch.cuda.synchronize()
        assert torch.isnan(buf).all(), bad
    buf = torch.full((NSEQ * heads * L * L,), float('nan'), device=DEV)
    for q, dc, s, p in ((None, dctx, seg, buf), (qkv, None, seg, buf), (qkv, dctx, None, buf), (qkv, dctx, seg, None)):
        rc = lib.vlmo_attn_gradcam(hip._p(q), hip._p(dc), hip._p(s), NSEQ, None, hip._p(p), heads, 64 * heads, L, 0, L, 0, 0,
                                   SCALE, stream)
        assert rc < 0 and lib.vlmo_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()
    for bad_qkv, bad_dctx in ((qkv.float(), dctx), (qkv, dctx.float()), (qkv, dctx.cpu()), (qkv, dctx.t().contiguous().t())):
        with pytest.raises(ValueError):                         # device tensors must be the engine's bf16 rows
            attnmap.attention_gradcam(bad_qkv, bad_dctx, seg, NSEQ, L, heads)


def test_public_entry_point_allocates_and_matches():
    heads, L = 3, 70
    qkv, dctx, seg, tok_rows, M, g = _layout(L, heads, True, seed=21)
    km = _masks(L, tok_rows, M, g)['scattered']
    rel = _rel_factor(qkv, heads, tok_rows)
    refs, _ = _wants_and_bounds(qkv, dctx, seg, heads, L, km, rel)
    want_h, bound_h = refs['cam']
    got = attnmap.attention_gradcam(qkv, dctx, seg, NSEQ, L, heads, keymask=km, scale=SCALE, queries=(3, 40), head_mean=True)
    assert got.shape == (NSEQ, 1, 40, L) and got.dtype == torch.float32 and not got.requires_grad
    want = want_h.mean(1, keepdim=True)[:, :, 3:43]
    bound = (bound_h.mean(1, keepdim=True) + heads * U * want_h.abs().mean(1, keepdim=True))[:, :, 3:43]
    assert ((got.double() - want).abs() <= bound).all()
