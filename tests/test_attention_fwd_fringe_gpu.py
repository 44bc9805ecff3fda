"""The attention forward at 257 .. 288 tokens (csrc/attention.hip, attn_fwd1_kernel<true>): eight waves walk the eight
full query tiles over all nine key tiles; the <= 32 fringe queries are split over the waves by key tile, normalised
against the exact row maximum, and their P^T tiles cross LDS to two waves that form the fringe rows of ctx.

ctx and lse (and, through the unchanged backward run on this forward's lse and ctx, dq / dk / dv / the qv column sums)
against the fp64 reference of tests/attn_cases.py under its per-element bounds, the lse tolerance and the suite's
earlier floors (ac.assert_within; the bounds are derived there and in tests/test_attention_bounds_cpu.py).  heads = 2,
3 - 4 sequences per launch, NaN-filled outputs.  Every launch runs twice: ctx and lse must repeat bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from exploremultimodal_amd import hip  # noqa: E402
from tests import attn_cases as ac  # noqa: E402
from tests import attn_counter  # noqa: E402
from tests.test_attention_peaked_gpu import _run  # noqa: E402

DEV = 'cuda'
DROP = hip.drop_params(0.1, True)
HEADS = 2


def _checked(case, drop):
    """forward + backward twice, bitwise equal; everything inside its bound"""
    keep = case.keep(ac.DROP_SEED, DROP[0]) if drop else None
    ref = ac.reference(case, keep, DROP[1] if drop else 1.0)
    a = _run(case, DROP if drop else None, ac.DROP_SEED)
    b = _run(case, DROP if drop else None, ac.DROP_SEED)
    u = case.used
    assert torch.equal(a['ctx'][u].view(torch.int16), b['ctx'][u].view(torch.int16)), 'ctx differs between two runs'
    ok = ~ref['lse'].isnan()
    assert torch.equal(a['lse'][:, :ok.shape[1]][ok], b['lse'][:, :ok.shape[1]][ok]), 'lse differs between two runs'
    ac.assert_within(a, ref, case)
    return a, ref


@pytest.mark.parametrize('pattern,mask,drop', [('rise', 'tail', False), ('mixed', 'tile', True), ('flat', 'tile', True)])
@pytest.mark.parametrize('n', [257, 261, 272, 287, 288])
def test_fringe_lengths(n, pattern, mask, drop):
    """fringes of 1, 5 (the workload's; rows packed from a 64-row and a 197-row range), 16, 31 and 32 tokens.  'tile'
    masks key tile 2 and the keys n - 7 .. n - 3: fringe keys from 263 tokens on, the last keys of tile 7 below."""
    case = ac.Case(f'{pattern}-{n}', pattern, (n, n, n), HEADS, mask, drop, 77 + n, DEV)
    _checked(case, drop)


def _exact_masks(masks):
    def exact(s, n, d, gen):
        x = torch.randn(n, 3 * d, generator=gen)
        do = torch.randn(n, d, generator=gen)
        return x, do, masks[s](n)
    return exact


def _km(n, dead=(), only=None):
    km = torch.ones(n, dtype=torch.int32)
    if only is not None:
        km[:] = 0
        km[list(only)] = 1
    km[list(dead)] = 0
    return km


@pytest.mark.parametrize('drop', [False, True])
def test_key_masks(drop):
    """all fringe keys masked; only key 0 live; some fringe keys masked; a whole key tile among tiles 0 - 7 masked beside
    part of the fringe"""
    masks = [lambda n: _km(n, dead=range(256, n)), lambda n: _km(n, only=[0]), lambda n: _km(n, dead=[257, 260, n - 1]),
             lambda n: _km(n, dead=list(range(160, 192)) + list(range(270, 280)))]
    case = ac.Case('key-masks', 'exact', (261, 261, 272, 288), HEADS, 'none', drop, 31, DEV, exact=_exact_masks(masks))
    _checked(case, drop)


@pytest.mark.parametrize('drop', [False, True])
def test_short_sequences_in_a_fringe_launch_are_what_a_256_token_launch_gives(drop):
    """261 beside 64, 197 and 256 tokens: the launch within its bounds, and the three short sequences bit for bit what a
    launch of max_len = 256 over them alone writes (same dropout mask: mask_seq0 = 1)"""
    case = ac.Case('mixed-launch', 'mixed', (261, 64, 197, 256), HEADS, 'tail', drop, 5, DEV)
    got, ref = _checked(case, drop)
    M, d = case.M, case.d
    kw = dict(drop=DROP, seed=ac.DROP_SEED, mask_seq0=1) if drop else {}
    ctx = torch.full((M, d), float('nan'), device=DEV, dtype=torch.bfloat16)
    lse = torch.full((3 * HEADS, 256), float('nan'), device=DEV)
    hip.attn_fwd(case.qkv, case.seg[1:].contiguous(), 3, case.keymask, ctx, lse, HEADS, d, 256, ac.SCALE, **kw)
    torch.cuda.synchronize()
    for s in (1, 2, 3):
        rows, n = case.rows[s], case.lens[s]
        assert torch.equal(ctx[rows].view(torch.int16), got['ctx'][rows].view(torch.int16)), f'ctx of sequence {s}'
        for hd in range(HEADS):
            assert torch.equal(lse[(s - 1) * HEADS + hd, :n], got['lse'][s * HEADS + hd, :n]), f'lse of sequence {s}'
    assert ctx[case.rows[0]].isnan().all()


def test_dropout_positions_of_fringe_rows_and_fringe_columns():
    """q = 0 and 64 live keys whose v rows are the 64 unit vectors: ctx[i, c] = keep(i, key c) / (64 (1 - p)), so the
    zeros of ctx ARE the dropped positions.  Live keys: the whole fringe and keys of every full tile.  Every query row,
    fringe rows included, against the host replica of the counter hash (tests/attn_counter.py), in a launch whose mask
    index starts at sequence 3 (mask_seq0 = 3)."""
    lens = (261, 288, 261)
    live = [list(range(256, 261)) + [j for j in range(256) if j % 11 == 3 and not 100 <= j < 140] + list(range(100, 140)),
            list(range(256, 288)) + list(range(0, 256, 8)),
            list(range(256, 261)) + list(range(59))]
    assert all(len(set(v)) == 64 for v in live)

    def exact(s, n, d, gen):
        x = torch.randn(n, 3 * d, generator=gen)
        x[:, :d] = 0
        x[:, 2 * d:] = 0
        for hd in range(d // 64):
            for c, j in enumerate(live[s]):
                x[j, 2 * d + hd * 64 + c] = 1.0
        return x, torch.zeros(n, d), _km(n, only=live[s])

    case = ac.Case('drop-positions', 'exact', lens, HEADS, 'none', True, 3, DEV, exact=exact)
    M, d, seq0 = case.M, case.d, 3
    ctx = torch.full((M, d), float('nan'), device=DEV, dtype=torch.bfloat16)
    lse = torch.full((len(lens) * HEADS, 288), float('nan'), device=DEV)
    hip.attn_fwd(case.qkv, case.seg, len(lens), case.keymask, ctx, lse, HEADS, d, 288, ac.SCALE, drop=DROP,
                 seed=ac.DROP_SEED, mask_seq0=seq0)
    torch.cuda.synchronize()
    keep = attn_counter.keep_mask(ac.DROP_SEED, lens, HEADS, DROP[0], seq0=seq0)
    want = (torch.tensor(DROP[1], dtype=torch.float32) / 64).bfloat16().item()      # the kernels' inv_keep / l in fp32
    for s, rows in enumerate(case.rows):
        n = lens[s]
        for hd in range(HEADS):
            k = keep[s, hd, :n][:, live[s]].to(DEV)
            c = ctx[rows][:, hd * 64:hd * 64 + 64].float()
            assert torch.equal(c != 0, k), f'sequence {s} head {hd}: {int(((c != 0) != k).sum())} positions differ from the replica'
            assert torch.equal(c[k], torch.full_like(c[k], want)), f'sequence {s} head {hd}: a kept probability is not 1 / 64'
            drop_rate = 1 - k.float().mean().item()
            assert 0.07 < drop_rate < 0.13, drop_rate
