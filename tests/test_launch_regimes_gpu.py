"""Element-wise checks of the HIP kernels in the launch regimes the training step runs them in (VLMo-Base, B = 64:
16 704 packed rows), which the per-kernel tests of tests/test_kernels_gpu.py stay below: row-partial kernels whose
workgroup count is capped at VLMO_MAX_PARTIAL_BLOCKS = 512 (csrc/common.h), NT GEMMs with more tiles than the 256 CUs
and 48 K-tiles, the tile = -1 planner at the model's shapes, weight gradients that walk 262 K-tiles or split them 27
ways, attention with four workgroups per CU.

Operands are generated on the device; references are torch on the device in fp64 (matmul, layer_norm) or the fp32
per-sequence attention of tests/kernel_refs.py.  Every comparison is exact (small integers: products and fp32 sums are
exact, bf16 holds integers below 256) or one of the tolerance formulas the small-shape test of the same quantity uses;
the docstrings name the test they come from.  Each docstring derives the grid / rows per workgroup / tile and K-tile
counts of its shapes from the launcher it names."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from exploremultimodal_amd import hip  # noqa: E402
from tests import dropmask  # noqa: E402
from tests.kernel_refs import _attn_keep_mask, _attn_lse_close, _attn_ref, _close  # noqa: E402

DEV = 'cuda'
DROP = hip.drop_params(0.1, True)            # (thresh, inv_keep)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ints(lo, hi, shape, g, dtype=torch.float32):
    """uniform integers in [lo, hi] on the device"""
    return torch.randint(lo, hi + 1, shape, device=DEV, generator=g).to(dtype)


def _randn(shape, g, dtype=torch.float32):
    return torch.randn(shape, device=DEV, generator=g).to(dtype)


def _eq(got, ref, what):
    """exact comparison on the device against an fp64 reference"""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = got != ref                       # a NaN is a mismatch too
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())}/{bad.numel()} elements differ, first at {idx}: '
                             f'got {got[tuple(idx)].item()!r} ref {ref[tuple(idx)].item()!r}')


# =========================================================================== 1. row-partial kernels above the 512 cap
LN_SHAPES = [(4099, 128), (4099, 768), (16704, 128), (16704, 768)]


@pytest.fixture(scope='module', params=LN_SHAPES, ids=lambda p: f'M{p[0]}-d{p[1]}')
def ln_ops(request):
    """x, w, b of a LayerNorm at (M, d) with the fp64 statistics; shared by the LayerNorm tests of the shape, never
    written"""
    M, d = request.param
    g = _gen(M + d)
    x = _randn((M, d), g) * 2 + 0.5
    w, b = _randn((d,), g) * 0.1 + 1, _randn((d,), g) * 0.1
    xd = x.double()
    mean, rstd = xd.mean(1), (xd.var(1, unbiased=False) + 1e-12).rsqrt()
    return dict(M=M, d=d, x=x, w=w, b=b, mean=mean, rstd=rstd, y=F.layer_norm(xd, (d,), w.double(), b.double(), 1e-12))


def _ln_grads(ops, dy):
    """fp64 autograd of the LayerNorm under the cotangent dy -> dx, dw, db"""
    xr, wr, br = (ops[k].double().clone().requires_grad_(True) for k in ('x', 'w', 'b'))
    F.layer_norm(xr, (ops['d'],), wr, br, 1e-12).backward(dy.double())
    return xr.grad, wr.grad, br.grad


def test_layernorm_fwd_bwd_with_several_row_groups_per_workgroup(ln_ops):
    """vlmo_ln_fwd / vlmo_ln_bwd above 4096 rows.  ln_bwd_grid (csrc/layernorm.hip): rpb = ceil(M / 512) rounded up to
    the 4 waves.  M = 4099: rpb 12, 342 workgroups, every wave loops over three rows and the last workgroup has 7 rows
    (waves 0 - 2 two rows, wave 3 one).  M = 16 704: rpb 36, 464 full workgroups, nine rows per wave.  The forward runs
    min(ceil(M / 8), 8192) = 513 / 2088 workgroups, two rows in flight per wave.  Comparisons and bounds of
    test_layernorm_fwd_bwd (1 / 128 + 1e-2 on bf16 y; 1e-3 + 1e-3 |ref| on dx; 1e-3 sqrt(M) on dw / db) against fp64;
    an integer-valued dy (bf16, and fp32 through the row map) makes db an exact sum: torch.equal."""
    M, d, x, w, b = (ln_ops[k] for k in ('M', 'd', 'x', 'w', 'b'))
    g = _gen(7 * M + d)
    sq = math.sqrt(M)
    y = torch.full((M, d), float('nan'), device=DEV, dtype=torch.bfloat16)
    mean, rstd = torch.full((M,), float('nan'), device=DEV), torch.full((M,), float('nan'), device=DEV)
    hip.ln_fwd(x, w, b, y, mean, rstd, None, M, d, 1e-12)
    _close(y, ln_ops['y'], 1 / 128, 1e-2, 'ln fwd')
    _close(mean, ln_ops['mean'], 1e-5, 1e-5, 'ln mean')
    perm = torch.randperm(M, device=DEV, generator=g).int()
    y32 = torch.full((M, d), float('nan'), device=DEV)
    hip.ln_fwd(x, w, b, y32, mean, rstd, perm, M, d, 1e-12)
    _close(y32[perm.long()], ln_ops['y'], 1e-4, 1e-4, 'ln fwd f32 rowmap')
    # backward, bf16 dy and an incoming residual gradient
    dy, dres = _randn((M, d), g, torch.bfloat16), _randn((M, d), g)
    rdx, rdw, rdb = _ln_grads(ln_ops, dy)
    dx = torch.full((M, d), float('nan'), device=DEV)
    dw, db = torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
    hip.ln_bwd(dy, None, x, w, mean, rstd, dres, dx, dw, db, M, d)
    _close(dx, rdx + dres.double(), 1e-3, 1e-3, 'ln dx')
    _close(dw, rdw, 1e-3, 1e-3 * sq, 'ln dw')
    _close(db, rdb, 1e-3, 1e-3 * sq, 'ln db')
    # fp32 dy through the row map, no residual
    dy32 = torch.full((M, d), float('nan'), device=DEV)
    dy32[perm.long()] = dy.float()
    dx2 = torch.full((M, d), float('nan'), device=DEV)
    hip.ln_bwd(dy32, perm, x, w, mean, rstd, None, dx2, None, None, M, d)
    _close(dx2, rdx, 1e-3, 1e-3, 'ln dx rowmap')
    # integer dy: db = column sums of dy, |sum| <= 3 M < 2^24
    dyi = _ints(-3, 3, (M, d), g)
    rdx, rdw, rdb = _ln_grads(ln_ops, dyi)
    for what, dyk, rowmap in (('bf16', dyi.bfloat16(), None), ('fp32 rowmap', None, perm)):
        if dyk is None:
            dyk = torch.full((M, d), float('nan'), device=DEV)
            dyk[perm.long()] = dyi
        dx3 = torch.full((M, d), float('nan'), device=DEV)
        dw3, db3 = torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
        hip.ln_bwd(dyk, rowmap, x, w, mean, rstd, None, dx3, dw3, db3, M, d)
        _close(dx3, rdx, 1e-3, 1e-3, f'ln dx, integer dy ({what})')
        _close(dw3, rdw, 1e-3, 1e-3 * sq, f'ln dw, integer dy ({what})')
        _eq(db3, rdb, f'ln db, integer dy ({what})')


@pytest.mark.parametrize('M,d', LN_SHAPES)
def test_resid_bwd_with_several_row_groups_per_workgroup(M, d):
    """vlmo_resid_bwd above 4096 rows.  resid_bwd_launch (csrc/elementwise.hip): block (d / 4, ry) with ry = min(4,
    1024 / (d / 4)) = 4 at d = 128 and 768, rpb = rows_per_block_for(M, 512, 2 ry) = ceil(M / 512) rounded up to 8:
    M = 4099 -> rpb 16, 257 workgroups, the last with 3 rows; M = 16 704 -> rpb 40, 418 workgroups, the last with 24.
    Integer dx, zd, gamma and row scales, no dropout: dz (|dz| <= 12, exact in bf16), dgamma and dbias (|sum| <= 12 M
    < 2^24) are exact, with the scale per row and through row_index.  With dropout: the replicated mask of
    tests/dropmask.py, bounds of test_resid_bwd_and_one_segment_ln_resid_bwd (dz one bf16 rounding: 1 / 128 relative +
    1e-6; the sums 1e-3 + 1e-3 sqrt(M))."""
    g = _gen(3 * M + d)
    dx, zd, gamma = _ints(-3, 3, (M, d), g), _ints(-2, 2, (M, d), g, torch.bfloat16), _ints(-2, 2, (d,), g)
    table = torch.tensor([0.0, 1, 2, 0, 1, 2, 1], device=DEV)
    ridx = _ints(0, 6, (M,), g, torch.int32)
    rows = table[ridx.long()]
    z = lambda *s: torch.zeros(*s, device=DEV)
    pre = dx.double() * gamma.double() * rows.double()[:, None]
    rdg = (dx.double() * rows.double()[:, None] * zd.double()).sum(0)
    for what, scale, index in (('row_index', table, ridx), ('scale per row', rows.contiguous(), None)):
        dz, dg, db = torch.full((M, d), float('nan'), device=DEV, dtype=torch.bfloat16), z(d), z(d)
        hip.resid_bwd(dx, zd, gamma, scale, dz, dg, db, M, d, row_index=index)
        _eq(dz, pre, f'resid_bwd dz ({what})')
        _eq(dg, rdg, f'resid_bwd dgamma ({what})')
        _eq(db, pre.sum(0), f'resid_bwd dbias ({what})')
    seed = 0x1234567ABCDEF01 + M
    keep = dropmask.keep_mask(seed, M, d, DROP[0]).to(DEV)          # host replica of the element dropout mask
    rdz = pre * keep * DROP[1]
    dz, dg, db = torch.full((M, d), float('nan'), device=DEV, dtype=torch.bfloat16), z(d), z(d)
    hip.resid_bwd(dx, zd, gamma, table, dz, dg, db, M, d, drop=DROP, seed=seed, row_index=ridx)
    sq = math.sqrt(M)
    _close(dz, rdz, 1 / 128, 1e-6, 'resid_bwd dz (dropout)')
    _close(dg, rdg, 1e-3, 1e-3 * sq, 'resid_bwd dgamma (dropout)')
    _close(db, rdz.sum(0), 1e-3, 1e-3 * sq, 'resid_bwd dbias (dropout)')
    assert torch.equal((dz == 0) | (pre == 0), ~keep | (pre == 0)), 'dz is not zero exactly where the mask drops'


@pytest.mark.parametrize('drop', [0.0, 0.1])
def test_ln_resid_bwd_one_segment_equals_ln_bwd_then_resid_bwd(ln_ops, drop):
    """vlmo_ln_resid_bwd (one segment) = vlmo_ln_bwd followed by vlmo_resid_bwd on the dx it wrote, as
    test_ln_resid_bwd_equals_ln_bwd_then_resid_bwd asserts at M = 1000: dx and dz bit-identical (same arithmetic, same
    dropout stream), the four column sums equal up to summation order (rtol 1e-4, atol 1e-3).  Grids: the fused kernel
    and ln_bwd use ln_bwd_grid (rpb 12 / 342 workgroups at M = 4099, rpb 36 / 464 at 16 704), resid_bwd rpb 16 / 257
    and rpb 40 / 418: the fused kernel's row groups differ from those of both separate kernels."""
    M, d, x, w = (ln_ops[k] for k in ('M', 'd', 'x', 'w'))
    g = _gen(11 * M + d)
    mean, rstd = ln_ops['mean'].float(), ln_ops['rstd'].float()
    dy, dres = _randn((M, d), g, torch.bfloat16), _randn((M, d), g)
    zd, gamma = _randn((M, d), g, torch.bfloat16), torch.rand(d, device=DEV, generator=g)
    scale = torch.rand(7, device=DEV, generator=g) + 0.5
    ridx = _ints(0, 6, (M,), g, torch.int32)
    dp = hip.drop_params(drop, True)
    z = lambda *s: torch.zeros(*s, device=DEV)
    nan = lambda dt: torch.full((M, d), float('nan'), device=DEV, dtype=dt)
    dx0, dw0, db0, dz0, dg0, dpb0 = nan(torch.float32), z(d), z(d), nan(torch.bfloat16), z(d), z(d)
    hip.ln_bwd(dy, None, x, w, mean, rstd, dres, dx0, dw0, db0, M, d)
    hip.resid_bwd(dx0, zd, gamma, scale, dz0, dg0, dpb0, M, d, drop=dp, seed=5, row_index=ridx)
    dx1, dw1, db1, dz1, dg1, dpb1 = nan(torch.float32), z(d), z(d), nan(torch.bfloat16), z(d), z(d)
    hip.ln_resid_bwd(dy, x, w, mean, rstd, dres, dx1, dw1, db1, zd, gamma, scale, ridx, dz1, dg1, dpb1, M, d, drop=dp, seed=5)
    assert not torch.isnan(dx0).any() and not torch.isnan(dz0.float()).any()
    assert torch.equal(dx0, dx1) and torch.equal(dz0, dz1)
    for a, b_ in ((dw0, dw1), (db0, db1), (dg0, dg1), (dpb0, dpb1)):
        torch.testing.assert_close(a, b_, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize('B,T,lens', [(161, 9, None), (195, 5, [5] + [4] * 194)], ids=['rpb12', 'rpb8-overflows'])
def test_two_segment_ln_resid_bias_folds_above_the_workgroup_cap(B, T, lens):
    """The two-segment form of the fused kernel (ln_resid_seg_bwd has no entry point of its own) through StackFn, as
    test_two_segment_ln_resid_bias_folds_with_a_ragged_segment_boundary does at 78 rows: mini width (d = 128, 17 image
    tokens), block 0 has two experts under a block that fuses with it; fc2 bias gradients of both experts, one StackFn
    call per pass (the fused kernel: partial rows [0, nb0) fold into the text expert's gradient, [nb0, grid) into the
    image expert's) against one call per block (each expert's vlmo_resid_bwd folds its own rows); same seed, 1e-4 of the
    gradient's largest element (summation order only), the bound of that test.
    rpb12: B = 161, 9-token texts: 1449 + 2737 = 4186 rows; ln_bwd_grid: rpb = ceil(4186 / 512) = 9 -> 12, 121 + 229
    workgroups, nb0 = 121, the last workgroup of either segment short (9 and 1 rows).
    rpb8-overflows: B = 195 with text lengths 5, 4, 4, ... (txt_lens): 781 + 3315 = 4096 rows; rpb starts at 8, where
    98 + 415 = 513 workgroups exceed the 512 partial rows of the workspace, so the while loop steps to rpb 12: 66 + 277
    = 343, nb0 = 66, last workgroups of 1 and 3 rows."""
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
    P = synth.num_img_tokens(mc)
    nt, ni = sum(lens) if lens else B * T, B * P
    assert nt + ni > 4088 and nt % 12 and ni % 12 and P == 17
    if lens:            # the grid at rpb 8 is one workgroup too many
        assert nt + ni <= 4096 and (nt + 7) // 8 + (ni + 7) // 8 > 512
    g = torch.Generator().manual_seed(41)
    tmask = torch.ones(B, T, dtype=torch.int64)
    if lens:
        tmask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).long()
    kw = dict(img=torch.randn(B, 3, mc.img_size, mc.img_size, generator=g).to(DEV),
              txt=torch.randint(1000, mc.vocab_size, (B, T), generator=g).to(DEV),
              img_attn_masks=torch.ones(B, P, dtype=torch.int64, device=DEV), txt_attn_masks=tmask.to(DEV))
    if lens:
        kw['txt_lens'] = lens
    R = torch.randn(B, T + P, mc.embed_dim, generator=g).to(DEV)
    names = ['blocks.0.mlp.l.fc2.bias', 'blocks.0.mlp.v.fc2.bias']
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
            pg = dict(model.named_parameters())
            got[stack] = [pg[n].grad.detach().clone() for n in names]
    finally:
        engine.USE_STACK = old
    for n, a, b in zip(names, got[True], got[False]):
        err, top = (a - b).abs().max().item(), b.abs().max().item()
        print(n, 'max |stack - per block| =', err, 'largest element', top)
        assert top > 0
        assert err <= 1e-4 * top, (n, err, top)


@pytest.mark.parametrize('M', [8195, 16704])
def test_colsum_and_colwork_multi_above_their_row_caps(M):
    """Column sums of a bf16 matrix, N = 520 columns of ld = 528 (the pad columns hold NaN), integers in [-3, 3]:
    |sum| <= 3 M < 2^24, exact.  vlmo_colsum: rpb = rows_per_block_for(M, 512, 16) -- M = 8195: ceil(8195 / 512) = 17 ->
    32 rows, grid (2, 257), the last row block has 3 rows; M = 16 704: 33 -> 48 rows, grid (2, 348).  vlmo_colwork_multi
    kind 1: 32 slices from 2048 rows, rps = ceil(M / 32) rounded up to 16 -- 8195: 257 -> 272, 31 slices, the last with
    35 rows; 16 704: 522 -> 528, 32 slices, the last with 336 -- times gx = 2 workgroups per slice, and one kind-0 fold
    job (300 partial rows of 4 x 192 integer columns into four outputs: 8 slices x 12 workgroups) in the same launch."""
    g = _gen(M)
    N, ld, d = 520, 528, 192
    x = torch.full((M, ld), float('nan'), device=DEV, dtype=torch.bfloat16)
    x[:, :N] = _ints(-3, 3, (M, N), g, torch.bfloat16)
    want = x[:, :N].double().sum(0)
    out = torch.zeros(N, device=DEV)
    hip.colsum(x, out, M, N)
    _eq(out, want, 'colsum')
    ws = _ints(-5, 5, (300, 4 * d), g)
    o = [_ints(-9, 9, (d,), g) for _ in range(4)]
    o0 = [t.clone() for t in o]
    cs = torch.ones(N, device=DEV)
    hip.colwork_multi([(0, ws, 300, 4 * d, o, d), (1, x, M, N, [cs], N)])
    _eq(cs, 1 + want, 'colwork_multi kind 1')
    for k in range(4):
        _eq(o[k], o0[k].double() + ws[:, k * d:(k + 1) * d].double().sum(0), f'colwork_multi fold out{k}')


# =========================================================================== 2. NT GEMM
def _sparse_ints(rows, K, g, density):
    """sparse small integers as test_gemm_nt_tile4_small_integers draws them (bf16, on the device)"""
    hit = torch.rand(rows, K, device=DEV, generator=g) < density
    return (hit * torch.randint(-2, 3, (rows, K), device=DEV, generator=g)).bfloat16()


def _nt_operands(Ms, N, K, seed, density=0.05):
    """per group: A [M, K], B [N, K] sparse integers with a dense first column that breaks symmetries, acc = A B^T in
    fp64"""
    g = _gen(seed)
    out = []
    for q, M in enumerate(Ms):
        A, B = _sparse_ints(M, K, g, density), _sparse_ints(N, K, g, density)
        B[:, 0] = ((torch.arange(N, device=DEV) + q) % 3).bfloat16()
        A[:, 0] = (torch.arange(M, device=DEV) % 2 + 1).bfloat16()
        out.append((A, B, A.double() @ B.double().t()))
    return out


def _side(M, N):
    """the integer side operands of test_gemm_nt_column_edges_exact_integers, built on the device"""
    i, j = torch.arange(M, device=DEV)[:, None], torch.arange(N, device=DEV)[None]
    return dict(bias=(j[0] % 7 - 3).float(), prior=((i * 3 + j) % 11 - 5).float(), resid=((i + j * 2) % 9 - 4).float(),
                gamma=(j[0] % 3 - 1).float(), rs=(i[:, 0] % 3).float(), x=((i * 2 + j) % 5 - 2).float())


def _gelu_grad(x):
    a = x.double().clone().requires_grad_(True)
    F.gelu(a).sum().backward()
    return a.grad


class _Guarded:
    """an [M, N] output inside a NaN-filled [M + 2, N + 4] buffer: nothing outside [M, N] may be written"""

    def __init__(self, M, N, dtype, fill=None):
        self.M, self.N = M, N
        self.t = torch.full((M + 2, N + 4), float('nan'), dtype=dtype, device=DEV)
        if fill is not None:
            self.t[:M, :N] = fill.to(dtype)

    def real(self, what):
        t, M, N = self.t, self.M, self.N
        assert torch.isnan(t[M:]).all() and torch.isnan(t[:M, N:]).all(), f'{what}: written outside [M, N]'
        return t[:M, :N]


def _check_colpart(cp, want, M, what, exact=False):
    """the checks of test_gemm_nt_dgelu_column_partials on cp [ceil(M / 16) + 1, N] (NaN before the launch): the spare
    row untouched, every real row written, their fold = the column sums, every row all zeros or the sum of one or two
    consecutive 16-row blocks starting at its own"""
    nblk = (M + 15) // 16
    N = want.shape[1]
    assert torch.isnan(cp[nblk]).all(), f'{what}: partial rows beyond ceil(M/16) were written'
    assert not torch.isnan(cp[:nblk]).any(), f'{what}: a column partial was left unwritten or took a NaN'
    tot = want.sum(0)
    if exact:
        _eq(cp[:nblk].double().sum(0), tot, f'fold of the partials, {what}')
    else:
        _close(cp[:nblk].sum(0), tot, 2e-3, 2e-3 * tot.abs().max().item(), f'fold of the partials, {what}')
    pad = torch.zeros(nblk * 16 + 16 - M, N, device=DEV, dtype=want.dtype)
    ref16 = torch.cat([want, pad]).view(nblk + 1, 16, N).sum(1)
    one, two = ref16[:nblk], ref16[:nblk] + ref16[1:]
    tol = 2e-3 * torch.maximum(one.abs().amax(1), two.abs().amax(1)) + 1e-6
    row = cp[:nblk].double()
    ok = (row == 0).all(1) | ((row - one).abs().amax(1) <= tol) | ((row - two).abs().amax(1) <= tol)
    assert ok.all(), f'{what}: partial row {int((~ok).nonzero()[0])} is neither zero nor the sum of one or two 16-row blocks'


def _run_nt(kind, tile, groups, N, K):
    """One launch (vlmo_gemm_nt, or vlmo_gemm_nt_grouped for several groups) of epilogue `kind` on the integer operands
    `groups` = [(A, B, acc)] and its checks.  Exact wherever the result is an integer: the recipes of
    test_gemm_nt_column_edges_exact_integers (bias, f32, f32 + beta, resid); gelu / dgelu at the bounds of that test
    (u exact, h and the derivative 1 / 128 + 1e-2); gelu_saved / dgelu_saved are the forms csrc/block.hip launches
    (relu bit 2: the fc1 epilogue saves GELU'(u) in place of u -- bounds of test_gemm_nt_saved_gelu_derivative -- and
    the backward multiplies by the saved factor: an integer factor makes du and its column partials exact)."""
    outs, kws, checks = [], [], []
    for q, (A, B, acc) in enumerate(groups):
        M = A.shape[0]
        s = _side(M, N)
        what = f'{kind}, tile {tile}, group {q}'
        ref = acc + s['bias'].double()
        assert ref.abs().max() < 256
        o = _Guarded(M, N, torch.float32 if kind in ('f32', 'f32_beta', 'resid') else torch.bfloat16,
                     s['prior'] if kind == 'f32_beta' else None)
        kw = dict(bias=s['bias'])
        if kind == 'bias':
            checks.append(lambda o=o, ref=ref, what=what: _eq(o.real(what), ref, what))
        elif kind == 'bias_none':
            kw = {}
            assert acc.abs().max() < 256
            checks.append(lambda o=o, acc=acc, what=what: _eq(o.real(what), acc, what))
        elif kind == 'f32':
            checks.append(lambda o=o, ref=ref, what=what: _eq(o.real(what), ref, what))
        elif kind == 'f32_beta':
            kw['beta'] = 1.0
            checks.append(lambda o=o, ref=ref, s=s, what=what: _eq(o.real(what), ref + s['prior'].double(), what))
        elif kind == 'resid':
            zd, resid = _Guarded(M, N, torch.bfloat16), _Guarded(M, N, torch.float32, s['resid'])
            kw.update(out2=zd.t, gamma=s['gamma'], resid=resid.t, row_scale=s['rs'])

            def chk(o=o, zd=zd, ref=ref, s=s, what=what):
                _eq(zd.real(what + ' zd'), ref, what + ' zd')
                _eq(o.real(what + ' out'), s['resid'].double() + s['gamma'].double() * ref * s['rs'].double()[:, None],
                    what + ' out')
            checks.append(chk)
        elif kind in ('gelu', 'gelu_saved'):
            h = _Guarded(M, N, torch.bfloat16)
            kw.update(out2=h.t)
            if kind == 'gelu_saved':
                kw.update(relu=4)

            def chk(o=o, h=h, ref=ref, what=what, saved=kind == 'gelu_saved'):
                if saved:
                    _close(o.real(what + ' saved derivative'), _gelu_grad(ref), 1 / 128, 1e-2, what + ' saved derivative')
                else:
                    _eq(o.real(what + ' u'), ref, what + ' u')
                _close(h.real(what + ' h'), F.gelu(ref), 1 / 128, 1e-2, what + ' h')
            checks.append(chk)
        else:               # dgelu, dgelu_saved: no bias, aux = the pre-activation or the saved factor
            aux = _Guarded(M, N, torch.bfloat16, s['x'])
            cp = torch.full(((M + 15) // 16 + 1, N), float('nan'), device=DEV)
            kw = dict(aux=aux.t, colpart=cp)
            saved = kind == 'dgelu_saved'
            if saved:
                kw.update(relu=4)
            want = acc * (s['x'].double() if saved else _gelu_grad(s['x']))
            if saved:
                assert want.abs().max() < 256

            def chk(o=o, cp=cp, want=want, M=M, what=what, saved=saved):
                if saved:
                    _eq(o.real(what), want, what)
                else:
                    _close(o.real(what), want, 1 / 128, 1e-2, what)
                _check_colpart(cp, want, M, what, exact=saved)
            checks.append(chk)
        outs.append(o.t)
        kws.append(kw)
    epi = dict(bias=hip.EPI_BIAS, bias_none=hip.EPI_BIAS, f32=hip.EPI_F32, f32_beta=hip.EPI_F32, resid=hip.EPI_RESID,
               gelu=hip.EPI_BIAS_GELU, gelu_saved=hip.EPI_BIAS_GELU, dgelu=hip.EPI_DGELU, dgelu_saved=hip.EPI_DGELU)[kind]
    if len(groups) == 1:
        A, B, _ = groups[0]
        hip.gemm_nt(epi, A, B, A.shape[0], N, K, outs[0], tile=tile, **kws[0])
    else:
        hip.gemm_nt_grouped(epi, [a for a, _, _ in groups], [b for _, b, _ in groups], [a.shape[0] for a, _, _ in groups],
                            N, K, outs, per_group=kws, tile=tile)
    for c in checks:
        c()


CHIP = (4355, 4100, 3072)
CHIP_KINDS = ([('bias', t) for t in (0, 3, 4, 8, 309, 313, 316, 320)] + [(k, t) for t in (0, 3) for k in ('f32', 'f32_beta')]
              + [('resid', t) for t in (0, 3, 8, 313, 320)] + [('gelu', t) for t in (0, 3, 4, 8, 313, 320)]
              + [('dgelu', t) for t in (0, 3, 8, 313, 320)])


@pytest.fixture(scope='module')
def chip_ops():
    """operands and fp64 product of the full-chip shape: shared by its cases, never written"""
    return _nt_operands([CHIP[0]], CHIP[1], CHIP[2], seed=4355)


@pytest.mark.parametrize('kind,tile', CHIP_KINDS, ids=[f'{k}-tile{t}' for k, t in CHIP_KINDS])
def test_gemm_nt_more_tiles_than_compute_units(chip_ops, kind, tile):
    """M = 4355, N = 4100, K = 3072: 48 K-tiles of 64 (the fc2 / fc1-dgrad depth of VLMo-Base); the weight is 25 MB, so
    group_m_for (csrc/gemm_nt.hip) = 4 and the 18 row panels of 256 form four groups of 4 and a ragged last group of 2;
    ragged edges in M (4355 = 17 x 256 + 3) and N (4100 = 16 x 256 + 4).  Tiles: 256 x 256 (tile 3): 18 x 17 = 306 > 256
    CUs, a second dispatch round; 128 x 128 (0): 35 x 33 = 1155; 256 x 128 (4): 18 x 33 = 594; 192 x 256 (8): 23 x 17 =
    391; (16 h) x 256 for 309 / 313 / 316 / 320: 31 / 21 / 18 / 14 row panels x 17 = 527 / 357 / 306 / 238.  Integer
    operands, every output an integer below 256: exact (_run_nt)."""
    M, N, K = CHIP
    _run_nt(kind, tile, chip_ops, N, K)


@pytest.fixture(scope='module', params=[1, 2, 3, 5, 36, 48], ids=lambda nk: f'nk{nk}')
def ktile_ops(request):
    """(300, 256, 64 nk) operands and fp64 product, shared by the tiles of a K-tile count; a fifth of the entries
    non-zero (|acc| stays below 256 at nk = 48: about 79 products of magnitude <= 4 per output)"""
    nk = request.param
    return nk, _nt_operands([300], 256, 64 * nk, seed=nk, density=0.2)


@pytest.mark.parametrize('tile', [0, 3, 4, 8, 313])
def test_gemm_nt_k_tile_counts(ktile_ops, tile):
    """(300, 256, 64 nk): 1 K-tile (the prologue's stage is all there is), 2, 3 and 5 (even and odd counts of the
    software-pipelined K loop), 36 and 48 (qkv-dgrad and fc2 depth of VLMo-Base; 48 also fc1-dgrad).
    Tiles: 128 x 128 -> 3 x 2 = 6 workgroups, 256 x 256 -> 2 x 1, 256 x 128 -> 2 x 2, 192 x 256 -> 2 x 1, 208 x 256
    (313) -> 2 x 1, the last row panel ragged in all of them.  Bias epilogue, integers, exact."""
    nk, groups = ktile_ops
    _run_nt('bias', tile, groups, 256, 64 * nk)


def _block_launches(d):
    """(name, epilogue kind, N, K) of the NT launches of one block, forward then backward (csrc/block.hip block_fwd /
    block_bwd; hidden = 4 d): the FFN ones are grouped launches there"""
    return [('qkv', 'bias', 3 * d, d), ('proj', 'resid', d, d), ('fc1', 'gelu_saved', 4 * d, d), ('fc2', 'resid', d, 4 * d),
            ('fc2 dgrad', 'dgelu_saved', 4 * d, d), ('fc1 dgrad', 'bias_none', d, 4 * d), ('proj dgrad', 'bias_none', d, d),
            ('qkv dgrad', 'bias_none', d, 3 * d)]


MODEL_LAUNCHES = ([('base', (16704,)) + l for l in _block_launches(768)] + [('large', (8352,)) + l for l in _block_launches(1024)]
                  + [('base-text', (4096,)) + l for l in _block_launches(768)]
                  + [('base-two-experts', (4096, 12608)) + l for l in _block_launches(768)[2:6]])


@pytest.mark.parametrize('model,Ms,name,kind,N,K', MODEL_LAUNCHES, ids=[f'{l[0]}-{l[2].replace(" ", "_")}' for l in MODEL_LAUNCHES])
def test_gemm_nt_planner_at_the_model_s_launches(model, Ms, name, kind, N, K):
    """tile = -1 (run_nt, csrc/gemm_nt.hip) at every NT launch of a block, with the epilogue forms csrc/block.hip uses
    (fc1 saves GELU'(u); the backward BIAS launches carry no bias; the DGELU launch leaves column partials).
    t256 = ceil(M / 256) ceil(N / 256) tiles of 256 x 256 decide the first pick; every shape here has N, K >= 512 and
    M N >= 40 x 65536, so the 16 x 16 x 32 heights h = 9 .. 20 then compete (rounds of 256 tiles x (h + 26)) and win
    when within 6 % of the first pick's cost.  Following the code by hand (first pick -> tile run, its tile count):
    base, M = 16 704: N = 768 (proj, fc2, the three d-wide dgrads; K = 768 / 2304 / 3072): t256 198, tile 3 -> 313,
    81 x 3 = 243 tiles, one round; qkv N = 2304: t256 594, tile 4 -> 319, 55 x 9 = 495, two rounds; fc1 / fc2 dgrad
    N = 3072: t256 792, tile 4 (gelu) or 0 (dgelu) -> 317, 62 x 12 = 744, three rounds.
    large, M = 8 352: N = 1024 (K = 1024 / 3072 / 4096): t256 132, 192-row tiles 44 x 4 = 176 fill 192 <= 0.9 x 256:
    tile 8 -> 309, 58 x 4 = 232; qkv N = 3072: t256 396, tile 4 -> 313, 41 x 12 = 492; N = 4096: t256 528, tile 8 ->
    317, 31 x 16 = 496.
    base-text, M = 4096: N = 768: t256 48 <= 128 (few_tiles) -> tile 0 whatever K, 32 x 6 = 192 tiles of 128 x 128, no
    16 x 16 x 32 height within 6 %; qkv N = 2304: t256 144, tile 3 -> 310, 26 x 9 = 234; N = 3072: t256 192, tile 3
    -> 313, 20 x 12 = 240.
    base-two-experts: the grouped FFN launches below the fusion layer, 4096 text rows + 12 608 image rows; the
    groups' row panels are counted apart (N = 768: 20 + 61 panels of 208 rows = 243 tiles; N = 3072: 16 + 47 panels
    of 272 = 756), each group's last panel ragged.  Integer operands; outputs exact, GELU-type outputs at the bounds
    _run_nt names."""
    _run_nt(kind, -1, _nt_operands(list(Ms), N, K, seed=N + K + Ms[0]), N, K)


# =========================================================================== 3. weight gradients (TN)
def _tn_problem(g, M, N1, N2, acc, alpha=None, extra=(64, 8, 4)):
    """integer problem with leading dimensions larger than the used columns -> (tuple for hip.gemm_tn_multi, fp64 ref)"""
    A, B = _ints(-2, 2, (M, N1 + extra[0]), g, torch.bfloat16), _ints(-2, 2, (M, N2 + extra[1]), g, torch.bfloat16)
    B[:, 0] += (torch.arange(M, device=DEV) % 3).bfloat16()
    C = _ints(-4, 4, (N1, N2 + extra[2]), g)
    ref = C.double().clone()
    prod = (alpha if alpha is not None else 1.0) * (A[:, :N1].double().t() @ B[:, :N2].double())
    ref[:, :N2] = prod + (ref[:, :N2] if acc else 0)
    return (A, B, C, M, N1, N2, acc) + ((alpha,) if alpha is not None else ()), ref


def _tn_run(probs):
    hip.gemm_tn_multi([p for p, _ in probs])
    for q, (p, ref) in enumerate(probs):
        _eq(p[2], ref, f'problem {q} {p[3:]}')          # the pad columns of C included: they keep their start values


def test_gemm_tn_multi_no_split_walks_262_k_tiles():
    """The weight gradients of two VLMo-Base blocks in one call, M = 16 709 tokens: (768, 2304), (768, 768), (768, 3072),
    (3072, 768), twice.  plan_tn_multi (csrc/tn_multi_plan.h): 27 + 9 + 36 + 36 = 108 tiles of 256 x 256 per block, 216
    >= 192 -> no split: one launch, every tile owned by one workgroup that walks all ceil(16 709 / 64) = 262 K-tiles, the
    last of 5 tokens; mode TN_ACCUM (1) or TN_STORE (2) by the accumulate flag; grid 216 (27 per XCD).  Integers in
    [-2, 2] (+ 0 .. 2 in one column): |sum| <= 8 x 16 709 < 2^24, exact; lda / ldb / ldc larger than the used columns."""
    M = 16709
    shapes = [(768, 2304), (768, 768), (768, 3072), (3072, 768)] * 2
    accs = [True, False, True, False, False, True, False, True]
    plan = hip.gemm_tn_multi_plan([(M, n1, n2, a) for (n1, n2), a in zip(shapes, accs)])
    assert len(plan) == 1 and plan[0]['grid'] == 216
    assert plan[0]['problems'] == [(t, 1, 262, 1 if a else 2, 0) for t, a in zip([27, 9, 36, 36] * 2, accs)]
    g = _gen(16709)
    _tn_run([_tn_problem(g, M, n1, n2, a) for (n1, n2), a in zip(shapes, accs)])


@pytest.mark.parametrize('acc', [True, False])
def test_gemm_tn_multi_split_27_ways(acc):
    """One problem (16 709, 768, 768) alone: 9 tiles < 192 -> splits = min(256 / 9, 262 / 8) = 28, kt_per_split =
    ceil(262 / 28) = 10, so 27 splits (26 of 10 K-tiles and one of 2), 243 workgroups in a grid of 248 (31 per XCD), fp32
    atomics (mode 0), the non-accumulating output zeroed first.  Exact on integers."""
    M = 16709
    assert hip.gemm_tn_multi_plan([(M, 768, 768, acc)])[0]['problems'] == [(9, 27, 10, 0, 0 if acc else 1)]
    _tn_run([_tn_problem(_gen(27 + acc), M, 768, 768, acc)])


def test_gemm_tn_multi_split_text_set():
    """The weight gradients of a text-only block, M = 4099 (65 K-tiles, the last of 3 tokens): (768, 2304), (768, 768),
    (768, 3072) -> 27 + 9 + 36 = 72 tiles < 192 -> splits = min(256 / 72, 65 / 8) = 3, kt_per_split 22 (22 + 22 + 21),
    216 workgroups, atomics; the non-accumulating problem is zeroed first."""
    M = 4099
    shapes = [(768, 2304, True), (768, 768, False), (768, 3072, True)]
    plan = hip.gemm_tn_multi_plan([(M,) + s for s in shapes])
    assert len(plan) == 1 and plan[0]['problems'] == [(27, 3, 22, 0, 0), (9, 3, 22, 0, 1), (36, 3, 22, 0, 0)]
    g = _gen(4099)
    _tn_run([_tn_problem(g, M, *s) for s in shapes])


@pytest.mark.parametrize('N1,N2', [(768, 768), (128, 776)])
@pytest.mark.parametrize('force', [0, 1001, 2001, 2003])
def test_gemm_tn_deep_token_dimension(force, N1, N2):
    """vlmo_gemm_tn at M = 16 709 (262 K-tiles, the last of 5 tokens), slab path and then the atomic path on top of it,
    as test_gemm_tn_tile_variants_exact does at M = 700.  tn_plan (csrc/gemm_tn.hip): 1001 = 128 x 128 tiles (36 / 7),
    one workgroup per tile walks all 262; 2001 = 256 x 256 tiles (9 / 4), likewise; 2003 = 256 x 256 in 3 splits of 88,
    88 and 86; 0 = the launcher's choice: (768, 768) -> 128 x 128, 512 / 36 = 14 splits of 19 (the last 15), (128, 776) ->
    7 tiles, 512 / 7 = 73 -> 66 splits of 4 (the last 2).  Integers, |sum| <= 8 M < 2^24: exact."""
    M = 16709
    g = _gen(force + N1)
    A, B = _ints(-2, 2, (M, N1), g, torch.bfloat16), _ints(-2, 2, (M, N2), g, torch.bfloat16)
    A[:, 0] += (torch.arange(M, device=DEV) % 3).bfloat16()
    ref = A.double().t() @ B.double()
    C = torch.zeros(N1, N2, device=DEV)
    hip.gemm_tn(A, B, C, M, N1, N2, splits=force)
    _eq(C, ref, 'slab path')
    hip.gemm_tn(A, B, C, M, N1, N2, splits=force, slab=False)
    _eq(C, 2 * ref, 'atomic path on top')


def test_gemm_tn_multi_alpha():
    """VlmoTnProblem.alpha through hip.gemm_tn_multi's optional eighth tuple entry: +-0.5 and 2 (powers of two: exact on
    integers) in the three epilogues.  Owner path: five problems of 64 .. 300 tokens (shortest reduction 1 K-tile ->
    splits 1), modes TN_ACCUM / TN_STORE; split path: the three problems of
    test_gemm_tn_multi_split_token_dimension_exact_integers (2 splits each, atomics, one zeroed first); a problem
    without the entry keeps alpha = 1."""
    g = _gen(99)
    owner = [(300, 768, 3072, True, 0.5), (200, 3072, 768, False, -0.5), (130, 768, 768, True, 2.0), (257, 2304, 768, False, 2.0),
             (64, 1000, 264, True, None)]
    assert [p[3] for p in hip.gemm_tn_multi_plan([s[:4] for s in owner])[0]['problems']] == [1, 2, 1, 2, 1]
    _tn_run([_tn_problem(g, *s) for s in owner])
    split = [(2000, 256, 512, True, -0.5), (1333, 96, 264, False, 0.5), (3000, 512, 256, True, 2.0)]
    assert [p[1:] for p in hip.gemm_tn_multi_plan([s[:4] for s in split])[0]['problems']] == [(2, 16, 0, 0), (2, 11, 0, 1), (2, 24, 0, 0)]
    _tn_run([_tn_problem(g, *s) for s in split])


# =========================================================================== 4. attention with the chip full
def _attn_keep_mask_device(seed, nseq, heads, N, thresh):
    """_attn_keep_mask (tests/kernel_refs.py) in int64 torch arithmetic on the device, masked to 32 bits the same way:
    the host replica of [86, 12, 261, 261] takes gigabytes of uint64 temporaries.  The test checks it against the host
    replica on a few sequences."""
    m = 0xFFFFFFFF

    def h32(x):
        x = x ^ (x >> 16)
        x = (x * 0x7feb352d) & m
        x = x ^ (x >> 15)
        x = (x * 0x846ca68b) & m
        return x ^ (x >> 16)
    bh = torch.arange(nseq * heads, device=DEV, dtype=torch.int64).view(nseq, heads)
    lo, hi = seed & m, seed >> 32
    akey = (h32((lo ^ ((bh * 0x9E3779B9) & m)) & m) + hi) & m
    q = torch.arange(N, device=DEV, dtype=torch.int64)[None, None, :, None]
    key = torch.arange(N, device=DEV, dtype=torch.int64)[None, None, None, :]
    x = ((((q * 512 + key) & m) * 0x9E3779B1) + akey[:, :, None, None]) & m
    x = x ^ (x >> 15)
    x = (x * 0x7feb352d) & m
    return (x >> 16) >= thresh


def _full_chip_attention_case():
    """86 sequences of 12 heads: lengths 261 (packed from a 64-row text range and a 197-row image range, like a fused
    layer), 197, 256 and 64 in turn; the text ranges lie in front of everything else"""
    lens = [(261, 197, 256, 64)[i % 4] for i in range(86)]
    n_packed = sum(n == 261 for n in lens)
    seg, row = [], 64 * n_packed
    for i, n in enumerate(lens):
        if n == 261:
            seg.append([64 * (i // 4), 64, row, 197])
            row += 197
        else:
            seg.append([row, n, 0, 0])
            row += n
    M = row
    keymask = torch.ones(M, dtype=torch.int32)
    g = torch.Generator().manual_seed(86)
    for i, s in enumerate(seg):
        if i % 2 == 1:                                    # as _attn_case: a tail of the first range masked
            p0 = int(torch.randint(2, s[1], (1,), generator=g))
            keymask[s[0] + p0:s[0] + s[1]] = 0
        elif i % 8 == 0:                                  # text padding inside a packed sequence
            keymask[s[0] + 40:s[0] + 64] = 0
    s = seg[4]                                            # keys 250 .. 260 of a packed sequence: its whole fringe tile
    keymask[s[2] + 186:s[2] + 197] = 0
    return lens, torch.tensor(seg, dtype=torch.int32).to(DEV), keymask.to(DEV), M


@pytest.mark.parametrize('dropout', [False, True])
def test_attention_with_four_workgroups_per_compute_unit(dropout):
    """One launch of 86 sequences x 12 heads = 1032 workgroups (vlmo_attn_fwd / vlmo_attn_bwd: one per (sequence, head);
    256 CUs), d = 768, max_len 261: nt = 9 tiles, so the forward is launch_fwd1 and the backward launch_bwd1<true>
    (eight owners + the fringe steps for the ninth tile) for every sequence, the 64-token ones included.  Key masks as
    _attn_case plus one over a whole fringe tile; with dropout the probabilities take the replicated mask.  ctx, dqkv
    and the per-sequence qv column sums against _attn_ref at the bounds of
    test_attention_backward_nine_tile_sequences_in_a_mixed_launch."""
    heads, d = 12, 768
    lens, seg, keymask, M = _full_chip_attention_case()
    nseq, N = len(lens), max(lens)
    assert nseq * heads == 1032 and N == 261
    g = _gen(1032)
    qkv, dctx = _randn((M, 3 * d), g, torch.bfloat16), _randn((M, d), g, torch.bfloat16)
    drop, seed = (hip.drop_params(0.1, True), 0xABCDEF0123) if dropout else (None, 0)
    kw = dict(drop=drop, seed=seed) if drop else {}
    keep = None
    if drop:
        keep = _attn_keep_mask_device(seed, nseq, heads, N, drop[0])
        assert torch.equal(keep[:3].cpu(), _attn_keep_mask(seed, 3, heads, N, drop[0]))                 # every (q, key)
        assert torch.equal(keep[:, :, :24, :24].cpu(), _attn_keep_mask(seed, nseq, heads, 24, drop[0]))   # every (sequence, head)
    ctx = torch.full((M, d), float('nan'), device=DEV, dtype=torch.bfloat16)
    lse = torch.zeros(nseq * heads, 288, device=DEV)
    hip.attn_fwd(qkv, seg, nseq, keymask, ctx, lse, heads, d, N, 64 ** -0.5, **kw)
    ref_ctx, ref_dqkv = _attn_ref(qkv, seg, keymask, heads, d, dctx, keep=keep, inv_keep=drop[1] if drop else 1.0)
    _close(ctx, ref_ctx, 1 / 64, 1e-2, 'attn ctx (full chip)')
    _attn_lse_close(lse, qkv, seg, keymask, heads, d, '(full chip)')
    dqkv = torch.full((M, 3 * d), float('nan'), device=DEV, dtype=torch.bfloat16)
    qv = torch.full((nseq, 2 * d), float('nan'), device=DEV)
    hip.attn_bwd(qkv, ctx, dctx, lse, seg, nseq, keymask, dqkv, heads, d, N, 64 ** -0.5, qv_colsum=qv, **kw)
    scale = ref_dqkv.abs().max().item()
    _close(dqkv, ref_dqkv, 1 / 32, 2e-2 * scale, 'attn dqkv (full chip)')
    for si, sg in enumerate(seg.tolist()):
        rows = torch.cat([torch.arange(sg[0], sg[0] + sg[1]), torch.arange(sg[2], sg[2] + sg[3])]).to(DEV)
        want = torch.cat([ref_dqkv[rows, :d].sum(0), ref_dqkv[rows, 2 * d:].sum(0)])
        _close(qv[si], want, 1 / 32, 2e-2 * scale * len(rows) ** 0.5, f'attn qv column sums (full chip, sequence {si})')


def test_attention_forward_577_tokens_twelve_heads():
    """Forward above 512 tokens (launch_fwd_long: K / V streamed): 12 sequences of 577 x 12 heads = 144 workgroups, d =
    768, lse stride 608; odd sequences have a masked tail.  ctx against _attn_ref at the bound of
    test_attention_fwd_bwd (1 / 64 + 1e-2)."""
    heads, d, nseq, N = 12, 768, 12, 577
    M = nseq * N
    g = _gen(577)
    qkv = _randn((M, 3 * d), g, torch.bfloat16)
    seg = torch.tensor([[i * N, N, 0, 0] for i in range(nseq)], dtype=torch.int32).to(DEV)
    keymask = torch.ones(M, dtype=torch.int32)
    for i in range(1, nseq, 2):
        keymask[i * N + 300 + 20 * i:(i + 1) * N] = 0
    keymask = keymask.to(DEV)
    ctx = torch.full((M, d), float('nan'), device=DEV, dtype=torch.bfloat16)
    lse = torch.full((nseq * heads, 608), float('nan'), device=DEV)
    hip.attn_fwd(qkv, seg, nseq, keymask, ctx, lse, heads, d, N, 64 ** -0.5)
    _close(ctx, _attn_ref(qkv, seg, keymask, heads, d), 1 / 64, 1e-2, 'attn ctx (577 tokens)')
