"""attnmap.attention_gradcam_reference, the torch statement of the gradient-weighted attention maps the HIP kernel
(vlmo_attn_gradcam) is held against: its G is what torch autograd leaves in ``P.grad`` of a hand-written attention
ctx = P v under the loss sum(ctx * dctx), and it follows the zero rules, the query window, the head mean and the kinds of
exploremultimodal_amd/attnmap.py.  No GPU."""
import pytest
import torch

from exploremultimodal_amd import attnmap, hip

KINDS = ('cam', 'attn_grad', 'grad')


def _case(L, heads, two_range, seed):
    """Packed qkv / dctx in fp64, 3 sequences (the middle one shorter than L; in the two-range form the second range
    lies before the first in memory) -> qkv, dctx, seg, the rows of every sequence's tokens."""
    lens = [L, max(1, L - 2), L]
    seg, tok_rows, row = [], [], 1
    for n in lens:
        len_a = n - n // 3 if two_range else n
        len_b = n - len_a
        row_b = row
        row += len_b + 2
        row_a = row
        row += len_a + 1
        seg.append([row_a, len_a, row_b if len_b else 0, len_b])
        tok_rows.append(torch.cat([torch.arange(row_a, row_a + len_a), torch.arange(row_b, row_b + len_b)]))
    M = row + 2
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(M, 3 * 64 * heads, generator=g, dtype=torch.float64)
    dctx = torch.randn(M, 64 * heads, generator=g, dtype=torch.float64)
    return qkv, dctx, torch.tensor(seg, dtype=torch.int32), tok_rows, M, g


def _masks(L, tok_rows, M, g):
    tail = torch.ones(M, dtype=torch.int32)
    tail[tok_rows[0][L - L // 3:]] = 0
    scat = (torch.rand(M, generator=g) >= 0.3).to(torch.int32)
    scat[tok_rows[1][0]] = 1                        # keep one key of every sequence: the all-masked rule has its own test
    scat[tok_rows[0][0]] = 1
    scat[tok_rows[2][0]] = 1
    return {'none': None, 'tail': tail if L >= 3 else None, 'scattered': scat}


def _autograd(qkv, dctx, rows, heads, valid, scale=0.125):
    """Hand-written attention of one sequence: leaf P = softmax(...) with retain_grad, ctx = P v, loss = sum(ctx * dctx)
    -> (P [heads, n, n], P.grad)."""
    d, n = 64 * heads, rows.numel()
    x = qkv[rows]
    q, k, v = (x[:, i * d:(i + 1) * d].reshape(n, heads, 64).transpose(0, 1) for i in range(3))
    s = (q @ k.transpose(-2, -1)) * scale
    if valid is not None:
        s = s.masked_fill(~valid[None, None, :], float('-inf'))
    s.requires_grad_(True)
    P = s.softmax(-1)
    P.retain_grad()
    ctx = (P @ v).transpose(0, 1).reshape(n, d)                 # head-major columns, as the engine's ctx
    (ctx * dctx[rows]).sum().backward()
    return P.detach(), P.grad


@pytest.mark.parametrize('L', [1, 5, 33])
@pytest.mark.parametrize('two_range', [False, True])
def test_reference_matches_autograd_of_a_hand_written_attention(L, two_range):
    heads = 2
    qkv, dctx, seg, tok_rows, M, g = _case(L, heads, two_range, seed=10 * L + two_range)
    for mname, km in _masks(L, tok_rows, M, g).items():
        for kind in KINDS:
            got = attnmap.attention_gradcam_reference(qkv, dctx, seg, 3, L, heads, keymask=km, scale=0.125, kind=kind,
                                                      dtype=torch.float64)
            assert got.shape == (3, heads, L, L) and got.dtype == torch.float64 and not torch.isnan(got).any()
            for s, rows in enumerate(tok_rows):
                n = rows.numel()
                valid = None if km is None else km[rows] != 0
                P, G = _autograd(qkv, dctx, rows, heads, valid)
                if valid is not None:
                    G = G * valid[None, None, :]                # zero rule of 'grad': autograd has dctx . v there
                want = {'grad': G, 'attn_grad': P * G, 'cam': P * G.clamp_min(0)}[kind]
                err = (got[s, :, :n, :n] - want).abs().max().item()
                assert err <= 1e-12 * max(1.0, want.abs().max().item()), (mname, kind, s, err)
                assert (got[s, :, n:] == 0).all() and (got[s, :, :, n:] == 0).all()


def _small(heads=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(40, 3 * 64 * heads, generator=g), torch.randn(40, 64 * heads, generator=g)


@pytest.mark.parametrize('kind', KINDS)
def test_zero_rules(kind):
    heads, L = 2, 12
    qkv, dctx = _small(heads)
    # sequence 0: rows 30..34 ++ 3..9 (12 tokens); 1: 7 tokens; 2: every key masked
    seg = torch.tensor([[30, 5, 3, 7], [12, 7, 0, 0], [20, 9, 0, 0]], dtype=torch.int32)
    km = torch.ones(40, dtype=torch.int32)
    km[20:29] = 0
    km[5] = 0                                                   # row 5 is token 7 of sequence 0
    X = attnmap.attention_gradcam_reference(qkv, dctx, seg, 3, L, heads, keymask=km, kind=kind, dtype=torch.float64)
    assert not torch.isnan(X).any()
    assert (X[0, :, :, 7] == 0).all()                           # a masked key
    assert (X[0, :, :, :7] != 0).any() and (X[0, :, 7, :7] != 0).any()      # the masked position as a QUERY is a row
    assert (X[1, :, 7:, :] == 0).all() and (X[1, :, :, 7:] == 0).all()      # past the sequence's own length
    assert (X[1, :, :7, :7] != 0).any()
    assert (X[2] == 0).all()                                    # every key masked: zeros for every kind


def test_kinds_are_consistent_and_a_fully_masked_launch_is_zero():
    heads, L = 2, 9
    qkv, dctx = _small(heads, seed=4)
    seg = torch.tensor([[0, 9, 0, 0], [10, 4, 20, 5]], dtype=torch.int32)
    P = attnmap.attention_probs_reference(qkv, seg, 2, L, heads, dtype=torch.float64)
    G, PG, cam = (attnmap.attention_gradcam_reference(qkv, dctx, seg, 2, L, heads, kind=k, dtype=torch.float64)
                  for k in ('grad', 'attn_grad', 'cam'))
    assert (PG - P * G).abs().max().item() <= 1e-15 and (cam - P * G.clamp_min(0)).abs().max().item() <= 1e-15
    assert (cam >= 0).all() and (G < 0).any()
    assert attnmap.attention_gradcam_reference(qkv, dctx, seg, 2, L, heads).equal(
        attnmap.attention_gradcam_reference(qkv, dctx, seg, 2, L, heads, kind='cam'))         # the default kind
    dead = torch.zeros(40, dtype=torch.int32)
    for k in KINDS:
        assert (attnmap.attention_gradcam_reference(qkv, dctx, seg, 2, L, heads, keymask=dead, kind=k) == 0).all()


@pytest.mark.parametrize('kind', KINDS)
def test_query_window_and_head_mean_are_slices_and_means(kind):
    heads, L = 3, 20
    g = torch.Generator().manual_seed(3)
    qkv, dctx = torch.randn(64, 3 * 64 * heads, generator=g), torch.randn(64, 64 * heads, generator=g)
    seg = torch.tensor([[0, 20, 0, 0], [40, 6, 20, 9]], dtype=torch.int32)
    km = (torch.arange(64) % 5 != 0).to(torch.int32)
    full = attnmap.attention_gradcam_reference(qkv, dctx, seg, 2, L, heads, keymask=km, kind=kind, dtype=torch.float64)
    mean = attnmap.attention_gradcam_reference(qkv, dctx, seg, 2, L, heads, keymask=km, kind=kind, head_mean=True,
                                               dtype=torch.float64)
    assert mean.shape == (2, 1, L, L) and torch.equal(mean, full.mean(1, keepdim=True))
    if kind != 'grad':      # the mean of the products, not the product of the means
        P = attnmap.attention_probs_reference(qkv, seg, 2, L, heads, keymask=km, head_mean=True, dtype=torch.float64)
        Gm = attnmap.attention_gradcam_reference(qkv, dctx, seg, 2, L, heads, keymask=km, kind='grad', head_mean=True,
                                                 dtype=torch.float64)
        assert (mean - P * (Gm.clamp_min(0) if kind == 'cam' else Gm)).abs().max().item() > 1e-3
    for q0, nq in ((0, 1), (5, 9), (19, 1), (0, 20)):
        for hm in (False, True):
            win = attnmap.attention_gradcam_reference(qkv, dctx, seg, 2, L, heads, keymask=km, kind=kind, queries=(q0, nq),
                                                      head_mean=hm, dtype=torch.float64)
            ref = (mean if hm else full)[:, :, q0:q0 + nq]
            assert win.shape == ref.shape and (win - ref).abs().max().item() <= 1e-13
    # CPU tensors take the restatement, in fp32
    a = attnmap.attention_gradcam(qkv, dctx, seg, 2, L, heads, keymask=km, kind=kind, queries=(5, 9), head_mean=True)
    b = attnmap.attention_gradcam_reference(qkv, dctx, seg, 2, L, heads, keymask=km, kind=kind, queries=(5, 9),
                                            head_mean=True)
    assert a.dtype == torch.float32 and a.equal(b)


@pytest.mark.parametrize('fn', [attnmap.attention_gradcam, attnmap.attention_gradcam_reference])
def test_argument_errors(fn):
    heads = 2
    qkv, dctx = torch.zeros(8, 3 * 64 * heads), torch.zeros(8, 64 * heads)
    seg = torch.tensor([[0, 8, 0, 0]], dtype=torch.int32)
    fn(qkv, dctx, seg, 1, 8, heads)
    for bad in (dict(heads=3), dict(seq_len=0), dict(seq_len=1025), dict(num_seq=0), dict(num_seq=2),
                dict(queries=(-1, 2)), dict(queries=(0, 0)), dict(queries=(4, 5)), dict(keymask=torch.ones(7, dtype=torch.int32)),
                dict(qkv=torch.zeros(8, 100)), dict(seg=torch.zeros(1, 3, dtype=torch.int32)),
                dict(kind='gradcam'), dict(kind=None), dict(dctx=torch.zeros(7, 64 * heads)), dict(dctx=torch.zeros(8, 64)),
                dict(dctx=torch.zeros(8, 3 * 64 * heads)), dict(dctx=torch.zeros(8 * 64 * heads))):
        kw = dict(qkv=qkv, dctx=dctx, seg=seg, num_seq=1, seq_len=8, heads=heads)
        kw.update(bad)
        with pytest.raises(ValueError):
            fn(**kw)


def test_text_to_image_heatmaps():
    B, H, T, grid = 2, 3, 4, 3
    N = T + 1 + grid * grid
    cam = torch.arange(B * H * N * N, dtype=torch.float32).reshape(B, H, N, N)
    hm = attnmap.text_to_image_heatmaps(cam, T, grid)
    assert hm.shape == (B, H, T, grid, grid)
    for t in range(T):
        for r in range(grid):
            for c in range(grid):
                assert torch.equal(hm[:, :, t, r, c], cam[:, :, t, T + 1 + r * grid + c])
    # a query window of the text rows and a head mean work the same way
    win = attnmap.text_to_image_heatmaps(cam[:, :1, :T], T, grid)
    assert win.shape == (B, 1, T, grid, grid) and torch.equal(win, hm[:, :1])
    for bad in (cam[:, :, :, :-1], cam[:, :, :T - 1], cam[0]):
        with pytest.raises(ValueError):
            attnmap.text_to_image_heatmaps(bad, T, grid)


def test_bindings():
    assert 'vlmo_attn_gradcam' in hip.exported_symbols()
    assert hip.GRADCAM_KINDS == {'cam': 0, 'attn_grad': 1, 'grad': 2}
    assert set(hip.GRADCAM_KINDS) == set(attnmap.KINDS)
