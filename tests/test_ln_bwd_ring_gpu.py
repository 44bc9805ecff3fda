"""ln_bwd_kernel with its rows waiting in a wave-private LDS ring (csrc/layernorm.hip, LnRing): every instantiation
the launchers reach -- bf16 dy with and without the residual branch, fp32 dy through a row map -- against an fp64 torch
restatement of the same formulas on the same inputs, at the bounds the LayerNorm tests already hold
(tests/test_kernels_gpu.py test_layernorm_fwd_bwd, tests/test_dropout_sites_gpu.py
test_resid_bwd_and_one_segment_ln_resid_bwd): fp32 outputs 1e-3 relative + 1e-3, column sums 1e-3 sqrt(M), dz one bf16
rounding (1 / 128) + dx's 1e-3 times the factor dx is multiplied by.

Shapes.  d = 192 (48 vectors: lanes 48-63 have no column, the pieces of a slot are shorter than one LDS-DMA
instruction), 768 (two slots of 10 KB per wave), 1024 (one slot per wave).  A workgroup takes rpb = max(8, ceil(M / 512)
rounded up to 4) rows, row r0 + wave + 4 k to wave `wave`:
  M = 1, 3, 4, 5       one workgroup, waves with 0 or 1 rows (and 2 at M = 5)
  M = 9, 13, 21        8-row workgroups and a ragged last one; 21 spans three
  M = 4099             rpb 12, 3 rows per wave: the ring wraps once; last workgroup 7 rows
  M = 8203             rpb 20, 5 rows per wave: the ring wraps twice and ends on an odd row; last workgroup 3 rows
Each case runs twice and must repeat bit for bit in what the kernel itself writes: dx, dz and its workgroups' partial
rows of the four column sums in the workspace.  (The fold that adds the partial rows into dw / db / dgamma / dbias uses
float atomics, several per address: its sums are held to the fp64 reference, not to each other.)"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from exploremultimodal_amd import hip  # noqa: E402
from tests import dropmask  # noqa: E402
from tests.kernel_refs import _close  # noqa: E402
from tests.test_dropout_sites_gpu import _check_mask  # noqa: E402

DEV = 'cuda'
DROP = hip.drop_params(0.1, True)
THRESH, INV = DROP
DS = [192, 768, 1024]
MS = [1, 3, 4, 5, 9, 13, 21, 4099, 8203]
SCALE = [0.0, 1 / 0.9, 1 / 0.9, 0.0, 1 / 0.9, 1 / 0.9, 1 / 0.9]


@functools.lru_cache(maxsize=2)
def _inputs(M, d):
    """the operands of a case, shared by its variants and never written"""
    g = torch.Generator().manual_seed(1000 * d + M)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    x = r(M, d) * 2 + 0.5
    t = dict(x=x, w=r(d) * 0.1 + 1, dy=r(M, d).bfloat16(), dres=r(M, d), mean=x.mean(1),
             rstd=(x.var(1, unbiased=False) + 1e-12).rsqrt(), zd=(r(M, d) + 0.3).bfloat16(), gamma=r(d),
             scale=torch.tensor(SCALE, device=DEV), ridx=torch.randint(0, 7, (M,), generator=g).to(torch.int32).to(DEV))
    t['rows'] = t['scale'][t['ridx'].long()]
    return t


def _reference(t, dy, dres, resid, keep):
    """fp64: dx = rstd (g - mean(g) - xh mean(g xh)) + dres with g = dy w, xh = (x - mean) rstd; dw = sum dy xh,
    db = sum dy; branch: dz = keep dx gamma rows / (1 - p), dgamma = sum dx rows zd, dbias = sum dz"""
    x, w, mean, rstd = (t[k].double() for k in ('x', 'w', 'mean', 'rstd'))
    dy = dy.double()
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * w
    dx = rstd[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    if dres is not None:
        dx = dx + dres.double()
    out = dict(dx=dx, dw=(dy * xh).sum(0), db=dy.sum(0))
    if resid:
        rows = t['rows'].double()[:, None]
        v = dx * t['gamma'].double() * rows
        if keep is not None:
            v = v * keep * INV
        out.update(dz=v, dgamma=(dx * rows * t['zd'].double()).sum(0), dbias=v.sum(0))
    return out


def _run(t, M, d, dy, rowmap, dres, resid, drop, seed):
    nan = lambda *s, dt=torch.float32: torch.full(s, float('nan'), device=DEV, dtype=dt)
    z = lambda: torch.zeros(d, device=DEV)
    out = dict(dx=nan(M, d), dw=z(), db=z())
    if resid:
        out.update(dz=nan(M, d, dt=torch.bfloat16), dgamma=z(), dbias=z())
        hip.ln_resid_bwd(dy, t['x'], t['w'], t['mean'], t['rstd'], dres, out['dx'], out['dw'], out['db'], t['zd'],
                         t['gamma'], t['scale'], t['ridx'], out['dz'], out['dgamma'], out['dbias'], M, d,
                         drop=drop, seed=seed)
    else:
        hip.ln_bwd(dy, rowmap, t['x'], t['w'], t['mean'], t['rstd'], dres, out['dx'], out['dw'], out['db'], M, d)
    # the launch's partial rows: ln_bwd_grid gives a workgroup rpb rows (one segment), hip.py hands over this scratch
    ncol = 4 if resid else 2
    rpb = max(8, (((M + 511) // 512 + 3) // 4) * 4)
    out['partials'] = hip.workspace(t['x'].device, ncol * d)[:(M + rpb - 1) // rpb * ncol * d].clone()
    return out


def _compare(what, got, ref, t, M, resid):
    sq = math.sqrt(M)
    tol = dict(dx=(1e-3, 1e-3), dw=(1e-3, 1e-3 * sq), db=(1e-3, 1e-3 * sq))
    if resid:
        amp_z = max(1.0, t['gamma'].abs().max().item() * t['rows'].max().item() * INV)
        amp_g = max(1.0, t['rows'].max().item() * t['zd'].float().abs().max().item())
        tol.update(dz=(1 / 128, 1e-3 * amp_z), dgamma=(1e-3, 1e-3 * sq * amp_g), dbias=(1e-3, 1e-3 * sq * amp_z))
    for k, (rt, at) in tol.items():
        err = (got[k].double() - ref[k]).abs().max().item()
        print(f'{what} {k}: max |err| {err:.3g} (atol {at:.3g}, rtol {rt:.3g})')
        _close(got[k], ref[k], rt, at, f'{what} {k}')


def _twice(what, t, M, d, *args):
    a, b = _run(t, M, d, *args), _run(t, M, d, *args)
    for k in ('dx', 'dz', 'partials'):
        if k in a:
            assert torch.equal(a[k], b[k]), f'{what} {k}: two runs differ'
    assert torch.isfinite(a['partials']).all()
    return a


@pytest.mark.parametrize('M', MS)
@pytest.mark.parametrize('d', DS)
def test_ln_bwd_ring(M, d):
    t = _inputs(M, d)
    seed = 0x1234567ABCDEF01 + M
    keep = dropmask.keep_mask(seed, M, d, THRESH).to(DEV)
    # fused with the residual branch, dropout on: every output, and the mask itself on the rows whose path is kept
    got = _twice('resid drop', t, M, d, t['dy'], None, t['dres'], True, DROP, seed)
    ref = _reference(t, t['dy'], t['dres'], True, keep)
    _compare('resid drop', got, ref, t, M, True)
    kept = t['rows'] != 0
    if kept.any():
        _check_mask(got['dz'][kept], (ref['dx'] * t['gamma'].double())[kept], keep[kept], 'resid drop dz')
    assert torch.equal(got['dz'][~kept], torch.zeros_like(got['dz'][~kept])), 'a dropped path has a gradient'
    # the same without dropout
    got = _twice('resid', t, M, d, t['dy'], None, t['dres'], True, (0, 1.0), 0)
    _compare('resid', got, _reference(t, t['dy'], t['dres'], True, None), t, M, True)
    # no branch: bf16 dy + incoming residual gradient
    got = _twice('plain', t, M, d, t['dy'], None, t['dres'], False, None, 0)
    _compare('plain', got, _reference(t, t['dy'], t['dres'], False, None), t, M, False)
    # fp32 dy read through a row map in reverse order, no residual gradient
    rev = torch.arange(M - 1, -1, -1, device=DEV, dtype=torch.int32)
    dy32 = torch.empty(M, d, device=DEV)
    dy32[rev.long()] = t['dy'].float()
    got = _twice('f32 rowmap', t, M, d, dy32, rev, None, False, None, 0)
    _compare('f32 rowmap', got, _reference(t, t['dy'], None, False, None), t, M, False)


def test_ln_bwd_rejects_a_width_the_ring_cannot_hold():
    """bf16 rows go to LDS in 16-byte units: d must be a multiple of 8"""
    t = _inputs(5, 192)
    with pytest.raises(Exception):
        hip.ln_bwd(t['dy'][:, :188].contiguous(), None, t['x'][:, :188].contiguous(), t['w'][:188].contiguous(),
                   t['mean'], t['rstd'], None, torch.empty(5, 188, device=DEV), None, None, 5, 188)


def test_two_segments_with_a_boundary_that_is_no_multiple_of_four():
    """The two-segment form (ln_resid_seg_bwd, reached through StackFn only) as
    test_two_segment_ln_resid_bias_folds_with_a_ragged_segment_boundary runs it, at B = 3 with 7-token texts: the
    boundary is row 21, the text segment's workgroups hold 8, 8 and 5 rows (waves with 2 / 1 / 1 / 1).  Stack path
    (the fused kernel) against the per-block path (vlmo_resid_bwd per expert), same seeds: 1e-4 of the gradient's
    largest element, the bound of that test (summation order only), on both experts' fc2 bias gradients."""
    from functools import partial
    from exploremultimodal_amd import engine
    from exploremultimodal_amd.vlmo import VLMO, LayerNorm
    from oracle import synth
    mc = synth.make_config('mini').model
    model = VLMO(img_size=mc.img_size, patch_size=mc.patch_size, in_chans=mc.in_chans, num_classes=mc.num_classes,
                 embed_dim=mc.embed_dim, depth=mc.depth, num_heads=mc.num_heads, mlp_ratio=mc.mlp_ratio,
                 qkv_bias=mc.qkv_bias, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.1,
                 norm_layer=partial(LayerNorm, eps=1e-12), init_values=mc.init_values, vocab_size=mc.vocab_size,
                 max_text_len=mc.max_text_len, fusion_layer=mc.fusion_layer)
    model.load_state_dict(synth.synth_backbone_state_dict(mc, 0, [('v', 'l', 'vl')] * mc.depth), strict=True)
    model = model.to(DEV).train()
    assert mc.fusion_layer == 1 and mc.depth == 2
    B, T, P = 3, 7, synth.num_img_tokens(mc)
    assert (B * T) % 4 and (B * P) % 4
    g = torch.Generator().manual_seed(43)
    kw = dict(img=torch.randn(B, 3, mc.img_size, mc.img_size, generator=g).to(DEV),
              txt=torch.randint(1000, mc.vocab_size, (B, T), generator=g).to(DEV),
              img_attn_masks=torch.ones(B, P, dtype=torch.int64, device=DEV),
              txt_attn_masks=torch.ones(B, T, dtype=torch.int64, device=DEV))
    R = torch.randn(B, T + P, mc.embed_dim, generator=g).to(DEV)
    names = ['blocks.0.mlp.l.fc2.bias', 'blocks.0.mlp.v.fc2.bias']
    pg = dict(model.named_parameters())
    got = {}
    old = engine.USE_STACK
    try:
        for stack in (True, False):
            engine.USE_STACK = stack
            for p in model.parameters():
                p.grad = None
            torch.manual_seed(5)
            x, _ = model.forward_features(**kw)
            (x * R).sum().backward()
            torch.cuda.synchronize()
            got[stack] = [pg[n].grad.detach().clone() for n in names]
    finally:
        engine.USE_STACK = old
    for n, a, b in zip(names, got[True], got[False]):
        err, top = (a - b).abs().max().item(), b.abs().max().item()
        print(n, 'max |stack - per block| =', err, 'largest element', top)
        assert top > 0
        assert err <= 1e-4 * top, (n, err, top)
