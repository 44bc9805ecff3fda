"""The training path's attention kernels (csrc/attention.hip) on scores that are not flat: rows whose maximum grows tile
after tile (the lazy rescale of attn_fwd1_kernel is taken eight times, alpha of the chunked and streaming forwards goes
to 1e-3), falls, does both inside one wave, sits on one key, or lies near -50; a whole masked tile in front.  The
smallest launches that reach each kernel:

    fwd1 / bwd1                          64, 256            chunked fwd / streaming bwd      289, 512
    fwd1 / bwd1 FRINGE                   257, 261, 288      streaming fwd / streaming bwd    513, 577

and two mixed launches.  Every case compares ctx, lse, dq, dk, dv and the qv column sums with the fp64 reference of
tests/attn_cases.py under its derived per-element bounds (and the earlier floors), asserts the premise the case exists
for, and starts from NaN-filled outputs.  The exact cases carry no tolerance at all.  Inputs, bounds and the CPU
counterpart (tests/test_attention_bounds_cpu.py): DESIGN.md 4p."""
import pytest
import torch

from exploremultimodal_amd import hip
from tests import attn_cases as ac

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DROP = hip.drop_params(0.1, True)
TABLE = dict(ac.case_table())


def _run(case, drop=None, seed=0):
    nseq, H, d, M, N = len(case.lens), case.heads, case.d, case.M, case.max_len
    kw = dict(drop=drop, seed=seed) if drop else {}
    ctx = torch.full((M, d), float('nan'), device=DEV, dtype=torch.bfloat16)
    lse = torch.full((nseq * H, ac.npad(N)), float('nan'), device=DEV)
    hip.attn_fwd(case.qkv, case.seg, nseq, case.keymask, ctx, lse, H, d, N, ac.SCALE, **kw)
    dqkv = torch.full((M, 3 * d), float('nan'), device=DEV, dtype=torch.bfloat16)
    qv = torch.full((nseq, 2 * d), float('nan'), device=DEV)
    hip.attn_bwd(case.qkv, ctx, case.dctx, lse, case.seg, nseq, case.keymask, dqkv, H, d, N, ac.SCALE, qv_colsum=qv, **kw)
    torch.cuda.synchronize()
    unused = torch.ones(M, dtype=torch.bool, device=DEV)
    unused[case.used] = False
    assert ctx[unused].isnan().all() and dqkv[unused].isnan().all(), 'a row of no sequence was written'
    return dict(ctx=ctx, lse=lse, dqkv=dqkv, qv=qv)


@pytest.mark.parametrize('name', list(TABLE))
def test_peaked_scores(name):
    kw = TABLE[name]
    case = ac.make_case(name, DEV, **kw)
    keep = case.keep(ac.DROP_SEED, DROP[0]) if kw['drop'] else None
    ref = ac.reference(case, keep, DROP[1] if kw['drop'] else 1.0)
    print(f'{name}: premises {ac.assert_premises(case, ref)}')
    got = _run(case, DROP if kw['drop'] else None, ac.DROP_SEED)
    ac.assert_within(got, ref, case)


@pytest.mark.parametrize('n', [261, 289, 513])
def test_one_live_key(n):
    """tile 0, the last full tile, the fringe: ctx is that key's v row bit for bit, dv its integer column sum"""
    case = ac.one_live_key_case(n, DEV)
    ac.check_one_live_key(_run(case), ac.reference(case), case)


def test_uniform_probabilities():
    """q = 0, 64 live keys among 261: ctx the exact mean, lse ln 64, dk zero, dv 2^-6 times the integer column sum"""
    case = ac.uniform_case(DEV)
    ac.check_uniform(_run(case), ac.reference(case), case)
