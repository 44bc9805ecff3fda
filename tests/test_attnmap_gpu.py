"""vlmo_attn_probs (the attention-map kernel) against attnmap.attention_probs_reference in fp64 on the same bf16 values.

Every launch writes into a NaN-filled buffer between two sentinel guard regions; every qkv row that belongs to no sequence
of the launch is NaN, so a read outside the segments or a write outside the output shows.

The bound is derived, not tuned.  Products of bf16 values are exact in fp32, so only the 64-term fp32 sum moves a score S,
by at most gamma = 64 u / (1 - 64 u) (u = 2^-24) times scale * sum |q_i| |k_i|; a score error e moves a probability by a
factor exp(e) on top and, through the row sum, on the bottom.  Required:

    |P - P64| <= (2 gamma scale max_ij (|q| @ |k|^T)_ij + 8 u) P64 + 1e-30

with the data-dependent factor computed here (about 1e-4 for these inputs); 8 u covers exp2, the division and the sums
of positive terms.  Where the definition says zero, P64 is zero and so must P be."""
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
LENGTHS = [1, 17, 32, 33, 64, 197, 261, 512, 513, 965, 1024]


def _layout(L, heads, two_range, seed):
    """qkv [M, 3d] bf16 with NaN outside the sequences, seg [3, 4], rows-of-token lists.  Sequence 1 is shorter than L;
    in the two-range form the second range lies BEFORE the first in memory."""
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
    used = torch.cat(tok_rows)
    qkv[used] = torch.randn(used.numel(), 3 * 64 * heads, generator=g)
    return qkv.bfloat16().to(DEV), torch.tensor(seg, dtype=torch.int32, device=DEV), tok_rows, M, g


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


def _launch(qkv, seg, nseq, km, heads, L, q0, nq, head_mean, scale=SCALE, d=None):
    """One kernel call into a guarded, NaN-filled buffer -> (status exception or None, output view, whole buffer)."""
    n = nseq * (1 if head_mean else heads) * nq * L
    buf = torch.full((GUARD + max(n, 0) + GUARD,), SENT, device=DEV)
    buf[GUARD:GUARD + n] = float('nan')
    out = buf[GUARD:GUARD + n]
    hip.attn_probs(qkv, seg, nseq, km, out, heads, 64 * heads if d is None else d, L, q0, nq, head_mean, scale)
    assert (buf[:GUARD] == SENT).all() and (buf[GUARD + n:] == SENT).all(), 'wrote outside probs'
    return out.view(nseq, 1 if head_mean else heads, nq, L)


def _bound_factor(qkv, heads, tok_rows):
    d = 64 * heads
    worst = 0.0
    for rows in tok_rows:
        x = qkv[rows.to(DEV)].float().abs()
        for h in range(heads):
            worst = max(worst, (x[:, 64 * h:64 * h + 64] @ x[:, d + 64 * h:d + 64 * h + 64].T).max().item())
    return 2 * GAMMA * SCALE * worst + 8 * U


@pytest.mark.parametrize('heads', [2, 3])
@pytest.mark.parametrize('L', LENGTHS)
def test_probs_match_fp64_reference(L, heads):
    report = []
    for two_range in (False, True):
        qkv, seg, tok_rows, M, g = _layout(L, heads, two_range, seed=1000 * heads + L)
        rel = _bound_factor(qkv, heads, tok_rows)
        assert rel < 5e-4
        for mname, km in _masks(L, tok_rows, M, g).items():
            ref = attnmap.attention_probs_reference(qkv, seg, NSEQ, L, heads, keymask=km, scale=SCALE, dtype=torch.float64)
            assert not torch.isnan(ref).any()
            ref_mean = ref.mean(dim=1, keepdim=True)
            for q0, nq in _windows(L):
                for head_mean in (False, True):
                    want = (ref_mean if head_mean else ref)[:, :, q0:q0 + nq]
                    got = _launch(qkv, seg, NSEQ, km, heads, L, q0, nq, head_mean)
                    assert not torch.isnan(got).any(), (two_range, mname, q0, nq, head_mean)
                    err = (got.double() - want).abs()
                    excess = (err - (rel * want + 1e-30)).max().item()
                    report.append((two_range, mname, q0, nq, head_mean, (err / (want + 1e-30)).max().item()))
                    print(f'L={L} H={heads} two_range={two_range} mask={mname} q=({q0},{nq}) mean={head_mean}: '
                          f'max rel err {report[-1][-1]:.3e} (bound {rel:.3e})')
                    assert excess <= 0, report[-1]
                    assert (got[want == 0] == 0).all()
            # zero rules, spelled out on the full map
            full = _launch(qkv, seg, NSEQ, km, heads, L, 0, L, False)
            n1 = tok_rows[1].numel()
            assert (full[1, :, n1:, :] == 0).all() and (full[1, :, :, n1:] == 0).all()
            if km is not None:
                for s in range(NSEQ):
                    dead = km[tok_rows[s].to(DEV)] == 0
                    assert (full[s][:, :, :dead.numel()][:, :, dead] == 0).all()
                    if bool(dead.all()):
                        assert (full[s] == 0).all()
            again = _launch(qkv, seg, NSEQ, km, heads, L, 0, L, False)
            assert torch.equal(full, again)
            a = _launch(qkv, seg, NSEQ, km, heads, L, 0, L, True)
            b = _launch(qkv, seg, NSEQ, km, heads, L, 0, L, True)
            assert torch.equal(a, b), 'head mean is not bitwise reproducible'


def test_lengths_in_seg_are_clamped_to_seq_len():
    """Whatever seg holds, nothing outside probs is written: lengths beyond seq_len and negative ones are clamped."""
    heads, L = 2, 40
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(300, 3 * 64 * heads, generator=g).bfloat16().to(DEV)
    seg = torch.tensor([[10, 90, 0, 0], [100, 30, 150, 70], [200, -4, 220, 25]], dtype=torch.int32, device=DEV)
    rel = _bound_factor(qkv, heads, [torch.arange(10, 50), torch.cat([torch.arange(100, 130), torch.arange(150, 160)]),
                                     torch.arange(220, 245)])
    for head_mean in (False, True):
        got = _launch(qkv, seg, 3, None, heads, L, 0, L, head_mean)
        ref = attnmap.attention_probs_reference(qkv, seg, 3, L, heads, scale=SCALE, head_mean=head_mean, dtype=torch.float64)
        assert not torch.isnan(got).any()
        assert ((got.double() - ref).abs() <= rel * ref + 1e-30).all()
        assert (got[2, :, 25:] == 0).all() and (got[2, :, :, 25:] == 0).all()


def test_refused_arguments_return_an_error_and_write_nothing():
    heads, L = 2, 33
    qkv, seg, tok_rows, M, g = _layout(L, heads, False, seed=9)
    good = dict(nseq=NSEQ, heads=heads, L=L, q0=0, nq=L, d=64 * heads)
    _launch(qkv, seg, NSEQ, None, heads, L, 0, L, False)
    for bad in (dict(d=64 * heads + 64), dict(d=32 * heads), dict(L=0), dict(L=1025), dict(q0=-1), dict(nq=0),
                dict(q0=1), dict(q0=L, nq=1), dict(nseq=0), dict(nseq=-1)):
        a = dict(good)
        a.update(bad)
        buf = torch.full((200000,), float('nan'), device=DEV)
        with pytest.raises(RuntimeError, match='vlmo_attn_probs'):
            hip.attn_probs(qkv, seg, a['nseq'], None, buf, a['heads'], a['d'], a['L'], a['q0'], a['nq'], False, SCALE)
        torch.cuda.synchronize()
        assert torch.isnan(buf).all(), bad
    lib = hip.lib()
    buf = torch.full((NSEQ * heads * L * L,), float('nan'), device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for q, s, p in ((None, seg, buf), (qkv, None, buf), (qkv, seg, None)):
        rc = lib.vlmo_attn_probs(hip._p(q), hip._p(s), NSEQ, None, hip._p(p), heads, 64 * heads, L, 0, L, 0, SCALE, stream)
        assert rc < 0 and lib.vlmo_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()
    with pytest.raises(ValueError):
        attnmap.attention_probs(qkv.float(), seg, NSEQ, L, heads)           # device tensors must be the engine's bf16 rows


def test_public_entry_point_allocates_and_matches():
    heads, L = 3, 70
    qkv, seg, tok_rows, M, g = _layout(L, heads, True, seed=21)
    km = _masks(L, tok_rows, M, g)['scattered']
    got = attnmap.attention_probs(qkv, seg, NSEQ, L, heads, keymask=km, queries=(3, 40), head_mean=True)
    ref = attnmap.attention_probs_reference(qkv, seg, NSEQ, L, heads, keymask=km, queries=(3, 40), head_mean=True,
                                            dtype=torch.float64)
    assert got.shape == (NSEQ, 1, 40, L) and got.dtype == torch.float32
    assert ((got.double() - ref).abs() <= _bound_factor(qkv, heads, tok_rows) * ref + 1e-30).all()
