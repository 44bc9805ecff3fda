"""attnmap.attention_probs_reference, the torch statement of the attention-map definition the HIP kernel is held against:
it equals the oracle's own soft-max (oracle.vlmo_oracle.attention) on the `small` preset's shapes, and follows the zero
rules, the query window and the head mean of exploremultimodal_amd/attnmap.py.  No GPU."""
import pytest
import torch

from exploremultimodal_amd import attnmap
from oracle import synth, vlmo_oracle

MC = synth.make_config('small').model
B, H, D = 3, MC.num_heads, MC.embed_dim


def _oracle_case(N, mask):
    """x [B, N, d] -> (packed qkv as the oracle forms it, seg, oracle attn [B, H, N, N])."""
    sd = synth.synth_backbone_state_dict(MC, 0)
    p = 'blocks.1.attn.'
    sd = dict(sd)
    sd[p + 'qkv.weight'] = sd[p + 'qkv.weight'] * 8.0          # peaked rows: a uniform map would hide a transpose
    x = torch.randn(B, N, D, generator=torch.Generator().manual_seed(N))
    _, attn = vlmo_oracle.attention(sd, p, x, mask, H)
    bias = torch.cat((sd[p + 'q_bias'], torch.zeros_like(sd[p + 'v_bias']), sd[p + 'v_bias']))
    qkv = torch.nn.functional.linear(x, sd[p + 'qkv.weight'], bias).reshape(B * N, 3 * D)
    seg = torch.tensor([[b * N, N, 0, 0] for b in range(B)], dtype=torch.int32)
    return qkv, seg, attn


@pytest.mark.parametrize('N', [MC.max_text_len, synth.num_img_tokens(MC), MC.max_text_len + synth.num_img_tokens(MC)])
@pytest.mark.parametrize('masked', [False, True])
def test_reference_equals_oracle_softmax(N, masked):
    mask = None
    if masked:
        mask = torch.ones(B, N, dtype=torch.int64)
        mask[1, N - 5:] = 0
        mask[2, 3::4] = 0
    qkv, seg, attn = _oracle_case(N, mask)
    km = mask.reshape(-1).to(torch.int32) if masked else None
    got = attnmap.attention_probs_reference(qkv, seg, B, N, H, keymask=km)
    assert got.shape == attn.shape == (B, H, N, N) and got.dtype == torch.float32
    # both are torch soft-max over the same fp32 scores: round-off of the batched against the per-sequence matmul
    assert (got - attn).abs().max().item() <= 1e-6
    assert (attn.max(-1).values > 4.0 / N).any()
    if masked:
        assert (got[1, :, :, N - 5:] == 0).all() and (got[2, :, :, 3::4] == 0).all()
        assert (got[1, :, N - 5:, :N - 5] > 0).all()        # a padded QUERY position is a row like any other
    assert attnmap.attention_probs(qkv, seg, B, N, H, keymask=km).equal(got)      # CPU tensors take the reference


def _packed(lens, rows, heads=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(rows, 3 * 64 * heads, generator=g)
    return qkv


def test_two_range_short_sequence_and_zero_rules():
    heads, L = 2, 12
    qkv = _packed(None, 40, heads)
    # sequence 0: rows 30..34 ++ 3..9 (12 tokens, the second range lies first in memory); 1: 7 tokens; 2: all masked
    seg = torch.tensor([[30, 5, 3, 7], [12, 7, 0, 0], [20, 9, 0, 0]], dtype=torch.int32)
    km = torch.ones(40, dtype=torch.int32)
    km[20:29] = 0
    km[5] = 0
    P = attnmap.attention_probs_reference(qkv, seg, 3, L, heads, keymask=km, dtype=torch.float64)
    assert P.dtype == torch.float64 and not torch.isnan(P).any()
    rows = torch.tensor([30, 31, 32, 33, 34, 3, 4, 5, 6, 7, 8, 9])
    x = qkv[rows].double()
    for h in range(heads):
        s = x[:, 64 * h:64 * h + 64] @ x[:, 128 + 64 * h:128 + 64 * h + 64].T * 0.125
        s[:, 7] = float('-inf')                                 # row 5 is token 7
        assert (P[0, h] - s.softmax(-1)).abs().max().item() <= 1e-12
    assert (P[0, :, :, 7] == 0).all()
    assert (P[1, :, 7:, :] == 0).all() and (P[1, :, :, 7:] == 0).all()       # past the sequence's own length
    assert (P[1, :, :7, :7].sum(-1) - 1).abs().max().item() <= 1e-12
    assert (P[2] == 0).all()                                    # every key masked: zeros, not NaN


def test_query_window_and_head_mean_are_slices_and_means():
    heads, L = 3, 20
    qkv = _packed(None, 64, heads, seed=3)
    seg = torch.tensor([[0, 20, 0, 0], [40, 6, 20, 9]], dtype=torch.int32)
    km = (torch.arange(64) % 5 != 0).to(torch.int32)
    full = attnmap.attention_probs_reference(qkv, seg, 2, L, heads, keymask=km)
    for q0, nq in ((0, 1), (5, 9), (19, 1), (0, 20)):
        win = attnmap.attention_probs_reference(qkv, seg, 2, L, heads, keymask=km, queries=(q0, nq))
        assert win.shape == (2, heads, nq, L)
        assert (win - full[:, :, q0:q0 + nq]).abs().max().item() <= 1e-7
        mean = attnmap.attention_probs_reference(qkv, seg, 2, L, heads, keymask=km, queries=(q0, nq), head_mean=True)
        assert mean.shape == (2, 1, nq, L)
        assert (mean - full[:, :, q0:q0 + nq].mean(1, keepdim=True)).abs().max().item() <= 1e-7
    s2 = attnmap.attention_probs_reference(qkv, seg, 2, L, heads, scale=0.25)
    assert (s2 - full).abs().max().item() > 1e-3                # the scale is used


@pytest.mark.parametrize('fn', [attnmap.attention_probs, attnmap.attention_probs_reference])
def test_argument_errors(fn):
    heads = 2
    qkv = torch.zeros(8, 3 * 64 * heads)
    seg = torch.tensor([[0, 8, 0, 0]], dtype=torch.int32)
    fn(qkv, seg, 1, 8, heads)
    for bad in (dict(heads=3), dict(seq_len=0), dict(seq_len=1025), dict(num_seq=0), dict(num_seq=2),
                dict(queries=(-1, 2)), dict(queries=(0, 0)), dict(queries=(4, 5)), dict(keymask=torch.ones(7, dtype=torch.int32)),
                dict(qkv=torch.zeros(8, 100)), dict(seg=torch.zeros(1, 3, dtype=torch.int32))):
        kw = dict(qkv=qkv, seg=seg, num_seq=1, seq_len=8, heads=heads)
        kw.update(bad)
        with pytest.raises(ValueError):
            fn(**kw)
