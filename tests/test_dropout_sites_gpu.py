"""Every kernel site of the element dropout hash (csrc/common.h drop_half / drop_bits4 / drop_keep) against a plain
fp64 torch reference of the same operation on the same bf16-rounded operands, with the keep mask taken from the host
replica tests/dropmask.py -- never from a kernel output.

Forward sites assert (a) the set of exactly-zero outputs equals ~keep element for element (elements whose reference
pre-dropout value is zero or rounds to zero in bf16 are left out; the inputs are gaussian with a non-zero bias so that
the reference leaves out none, which is asserted, cap 1e-4 of the elements) and (b) the survivors equal the reference
scaled by 1 / (1 - p) at the tolerance the dropout-off test of that kernel in tests/test_kernels_gpu.py uses.  Backward
sites compare the whole result with autograd through the reference forward under the same mask.

Index spaces checked here ("Dropout wiring"): the GEMM epilogues and vlmo_resid_bwd / vlmo_ln_resid_bwd
count rows from the first row of the matrix the launch (or the group of a grouped launch) is handed; the image
embedding counts (b * (npatch + 1) + t) * d + c; the text embeddings count packed rows.  The two-segment form of
vlmo_ln_resid_bwd (ln_resid_seg_bwd: seed0 / seed1, rows of the second segment counted from the segment boundary) is
internal to vlmo_stack_bwd and has no entry point of its own: tests/test_dropout_stack_gpu.py checks it in place
(case 'vl', 27 text rows + 51 image rows)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from exploremultimodal_amd import hip  # noqa: E402
from tests import dropmask  # noqa: E402
from tests.kernel_refs import _close, _rand  # noqa: E402

DEV = 'cuda'
P_DROP = 0.1
DROP = hip.drop_params(P_DROP, True)            # (thresh, inv_keep)
THRESH, INV = DROP
CAP = 1e-4                                      # share of the elements (a) may leave out
SHAPES = [(300, 256, 128), (77, 128, 192), (1000, 384, 768)]
TILES = [0, 3, 4, 313, 317, 110]
SEEDS = {300: 1234, 77: 0x1234567ABCDEF01, 1000: 2 ** 62 - 5}


def test_replica_parameters_are_the_library_s():
    assert dropmask.thresh_of(P_DROP) == DROP


@functools.lru_cache(maxsize=None)
def _keep(seed, M, N, row0=0):
    return dropmask.keep_mask(seed, M, N, THRESH, row0).to(DEV)


@functools.lru_cache(maxsize=None)
def _operands(M, N, K):
    """gaussian bf16 operands with a unit-variance product (so that GELU never underflows) and a bias that is nowhere
    zero; acc = A B^T + bias in fp64: shared by every test of the shape, never written"""
    A, B = _rand(M, K, seed=4 + M), _rand(N, K, scale=1 / math.sqrt(K), seed=5 + M)
    bias = _rand(N, seed=6 + M, dtype=torch.float32) * 0.1 + 0.3
    acc = A.double() @ B.double().t() + bias.double()
    return A, B, bias, acc


def _gelu_grad(u):
    a = u.clone().requires_grad_(True)
    F.gelu(a).sum().backward()
    return a.grad


def _left_out(pre):
    """reference side of condition (a): elements whose pre-dropout value is zero or rounds to zero in bf16"""
    out = pre.float().bfloat16() == 0
    n = int(out.sum())
    assert n <= CAP * pre.numel(), f'{n} of {pre.numel()} reference values are zero: choose other inputs'
    return out, n


def _check_mask(got, pre, keep, what):
    """(a): got == 0 exactly where ~keep"""
    out, n = _left_out(pre)
    bad = ((got == 0) != ~keep) & ~out
    print(f'{what}: {n} elements left out of the mask comparison, {int(bad.sum())} mismatches, '
          f'drop rate {1 - keep.float().mean().item():.4f}')
    if bad.any():
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())}/{bad.numel()} elements are zero where the replicated mask keeps them '
                             f'or the reverse, first at {idx} (keep {bool(keep[tuple(idx)])}, got {got[tuple(idx)].item()})')
    assert n == 0, f'{what}: the reference left out {n} elements (expected none)'


def _report(what, got, ref):
    err = (got.double() - ref.double()).abs().max().item()
    print(f'{what}: max |got - ref| = {err:.4g} (largest |ref| {ref.abs().max().item():.4g})')


# ------------------------------------------------------------------------------------------------ GEMM epilogues
@pytest.mark.parametrize('tile', TILES)
@pytest.mark.parametrize('M,N,K', SHAPES)
def test_resid_epilogue(tile, M, N, K):
    """VLMO_EPI_RESID: out2 = dropout(acc + bias), out = resid + gamma * out2 * row_scale, row scale per row and per
    group through row_index"""
    A, B, bias, acc = _operands(M, N, K)
    seed = SEEDS[M]
    keep = _keep(seed, M, N)
    resid = _rand(M, N, seed=7, dtype=torch.float32)
    gamma = _rand(N, seed=8, dtype=torch.float32)
    g = torch.Generator().manual_seed(M)
    ref_zd = acc * keep * INV
    for mode in ('row', 'group'):
        if mode == 'row':
            rs = ((torch.rand(M, generator=g) > 0.3).float() / 0.7).to(DEV)
            ridx, rows = None, rs
        else:
            rs = ((torch.rand(7, generator=g) > 0.3).float() / 0.7).to(DEV)
            ridx = torch.randint(0, 7, (M,), generator=g).to(torch.int32).to(DEV)
            rows = rs[ridx.long()]
        xo = torch.full((M, N), float('nan'), device=DEV)
        zd = torch.full((M, N), float('nan'), device=DEV, dtype=torch.bfloat16)
        hip.gemm_nt(hip.EPI_RESID, A, B, M, N, K, xo, out2=zd, bias=bias, gamma=gamma, resid=resid, row_scale=rs,
                    row_index=ridx, drop=DROP, seed=seed, tile=tile)
        _check_mask(zd, acc, keep, f'resid.out2 ({mode} scale)')
        _report('resid.out2', zd, ref_zd)
        _close(zd, ref_zd, 1 / 128, 1e-2, 'resid.out2 survivors')
        ref_out = resid.double() + gamma.double() * ref_zd * rows.double()[:, None]
        _report('resid.out', xo, ref_out)
        _close(xo, ref_out, 1e-3, 1e-3, f'resid.out ({mode} scale)')


@pytest.mark.parametrize('tile', TILES)
@pytest.mark.parametrize('M,N,K', SHAPES)
def test_gelu_epilogue_plain_and_saved_derivative(tile, M, N, K):
    """VLMO_EPI_BIAS_GELU.  Plain form: out = u, out2 = dropout(gelu(u)).  VlmoEpilogue.relu bit 2: out = GELU'(u) *
    mask / (1 - p) in place of u, out2 as before."""
    A, B, bias, acc = _operands(M, N, K)
    seed = SEEDS[M] + 20
    keep = _keep(seed, M, N)
    h_ref, d_ref = F.gelu(acc), _gelu_grad(acc)
    u = torch.full((M, N), float('nan'), device=DEV, dtype=torch.bfloat16)
    hh = torch.full_like(u, float('nan'))
    hip.gemm_nt(hip.EPI_BIAS_GELU, A, B, M, N, K, u, out2=hh, bias=bias, drop=DROP, seed=seed, tile=tile)
    _close(u, acc, 1 / 128, 1e-2, 'gelu.u')
    _check_mask(hh, h_ref, keep, 'gelu.out2')
    _report('gelu.out2', hh, h_ref * keep * INV)
    _close(hh, h_ref * keep * INV, 1 / 128, 1e-2, 'gelu.out2 survivors')
    g = torch.full_like(u, float('nan'))
    hh2 = torch.full_like(u, float('nan'))
    hip.gemm_nt(hip.EPI_BIAS_GELU, A, B, M, N, K, g, out2=hh2, bias=bias, relu=4, drop=DROP, seed=seed, tile=tile)
    _check_mask(hh2, h_ref, keep, 'gelu.out2 (saved-derivative form)')
    _check_mask(g, d_ref, keep, 'gelu.out = saved derivative')
    _report('saved derivative', g, d_ref * keep * INV)
    _close(hh2, h_ref * keep * INV, 1 / 128, 1e-2, 'gelu.out2 survivors (saved-derivative form)')
    _close(g, d_ref * keep * INV, 1 / 128, 1e-2, 'saved derivative survivors')


@pytest.mark.parametrize('tile', TILES)
@pytest.mark.parametrize('M,N,K', SHAPES)
def test_dgelu_epilogue_recomputing_and_saved(tile, M, N, K):
    """VLMO_EPI_DGELU = d/du of dropout(gelu(u)) under the incoming gradient acc.  Recomputing form: aux = u, the
    epilogue regenerates the mask.  Saved form: aux = the forward's saved GELU'(u) * mask / (1 - p)."""
    A, B, _, _ = _operands(M, N, K)
    acc = A.double() @ B.double().t()               # no bias in this epilogue
    seed = SEEDS[M] + 22
    keep = _keep(seed, M, N)
    aux = _rand(M, N, seed=9)
    want = acc * _gelu_grad(aux.double()) * keep * INV
    du = torch.full((M, N), float('nan'), device=DEV, dtype=torch.bfloat16)
    hip.gemm_nt(hip.EPI_DGELU, A, B, M, N, K, du, aux=aux, drop=DROP, seed=seed, tile=tile)
    _check_mask(du, acc * _gelu_grad(aux.double()), keep, 'dgelu (recomputing)')
    _report('dgelu (recomputing)', du, want)
    _close(du, want, 1 / 128, 1e-2, 'dgelu (recomputing)')
    # saved form, fed what the forward wrote for the same u and seed: A1 B1^T + bias = u up to the forward's rounding
    A1, B1, bias, u = _operands(M, N, K)
    g = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    hh = torch.empty_like(g)
    hip.gemm_nt(hip.EPI_BIAS_GELU, A1, B1, M, N, K, g, out2=hh, bias=bias, relu=4, drop=DROP, seed=seed, tile=tile)
    du2 = torch.full_like(du, float('nan'))
    hip.gemm_nt(hip.EPI_DGELU, A, B, M, N, K, du2, aux=g, relu=4, tile=tile)
    # the mask against the replica; the values against the epilogue's own bf16 operand g (which
    # test_gelu_epilogue_plain_and_saved_derivative holds to GELU'(u) * mask / (1 - p))
    _check_mask(du2, acc * _gelu_grad(u), keep, 'dgelu (saved)')
    _report('dgelu (saved)', du2, acc * g.double())
    _close(du2, acc * g.double(), 1 / 128, 1e-2, 'dgelu (saved)')


@pytest.mark.parametrize('tile', [0, 3, 317])
@pytest.mark.parametrize('epi', ['bias_gelu', 'resid'])
def test_grouped_launch_counts_rows_from_each_group_s_first_row(tile, epi):
    """vlmo_gemm_nt_grouped, two groups of unequal ragged heights (the text and image experts of a block below the
    fusion layer) with per-group seeds: group g's mask is keep_mask(seed_g, M_g, N), rows counted from ITS first row --
    not from the launch's."""
    Ms, N, K = [77, 300], 256, 128
    seeds = [0x5EED00000021, 0x5EED00000023]
    A300, B0, bias0, _ = _operands(300, N, K)
    As = [A300[:77].contiguous(), A300]
    Bs = [B0, _rand(N, K, scale=1 / math.sqrt(K), seed=99)]
    biases = [bias0, bias0 + 0.1]
    accs = [As[i].double() @ Bs[i].double().t() + biases[i].double() for i in range(2)]
    keeps = [_keep(seeds[i], Ms[i], N) for i in range(2)]
    if epi == 'bias_gelu':
        outs = [torch.full((m, N), float('nan'), device=DEV, dtype=torch.bfloat16) for m in Ms]
        per = [dict(bias=biases[i], out2=torch.full((Ms[i], N), float('nan'), device=DEV, dtype=torch.bfloat16),
                    seed=seeds[i]) for i in range(2)]
        hip.gemm_nt_grouped(hip.EPI_BIAS_GELU, As, Bs, Ms, N, K, outs, per_group=per, tile=tile, drop=DROP, relu=4)
        for i in range(2):
            _check_mask(per[i]['out2'], F.gelu(accs[i]), keeps[i], f'grouped gelu.out2, group {i}')
            _check_mask(outs[i], _gelu_grad(accs[i]), keeps[i], f'grouped saved derivative, group {i}')
            _close(per[i]['out2'], F.gelu(accs[i]) * keeps[i] * INV, 1 / 128, 1e-2, f'grouped gelu.out2, group {i}')
            _close(outs[i], _gelu_grad(accs[i]) * keeps[i] * INV, 1 / 128, 1e-2, f'grouped saved derivative, group {i}')
    else:
        gamma = _rand(N, seed=8, dtype=torch.float32)
        resids = [_rand(m, N, seed=30 + i, dtype=torch.float32) for i, m in enumerate(Ms)]
        rs = torch.tensor([0.0, 1 / 0.9, 1 / 0.9, 0.0, 1 / 0.9], device=DEV)
        ridx = [torch.arange(m, device=DEV, dtype=torch.int32) % 2 + 2 * i for i, m in enumerate(Ms)]
        outs = [torch.full((m, N), float('nan'), device=DEV) for m in Ms]
        per = [dict(bias=biases[i], resid=resids[i], row_index=ridx[i], seed=seeds[i],
                    out2=torch.full((Ms[i], N), float('nan'), device=DEV, dtype=torch.bfloat16)) for i in range(2)]
        hip.gemm_nt_grouped(hip.EPI_RESID, As, Bs, Ms, N, K, outs, per_group=per, tile=tile, drop=DROP, gamma=gamma,
                            row_scale=rs)
        for i in range(2):
            zd = accs[i] * keeps[i] * INV
            _check_mask(per[i]['out2'], accs[i], keeps[i], f'grouped resid.out2, group {i}')
            _close(per[i]['out2'], zd, 1 / 128, 1e-2, f'grouped resid.out2, group {i}')
            want = resids[i].double() + gamma.double() * zd * rs[ridx[i].long()].double()[:, None]
            _close(outs[i], want, 1e-3, 1e-3, f'grouped resid.out, group {i}')


# ------------------------------------------------------------------------------------------------ backward of the branch
class _RoundBf16(torch.autograd.Function):
    """the forward saves the dropped branch output in bf16; its gradient passes through"""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def _branch_reference(pre, bias, gamma, rows, keep, dx):
    """autograd through y = gamma * dropout(pre + bias) * row scale under the cotangent dx (fp64): the saved branch
    output zd (what the forward's out2 holds), d pre, d gamma, d bias"""
    pre, bias, gamma = (t.double().clone().requires_grad_(True) for t in (pre, bias, gamma))
    zd = _RoundBf16.apply((pre + bias) * keep * INV)
    y = gamma * zd * rows.double()[:, None]
    y.backward(dx.double())
    return zd.detach(), pre.grad, gamma.grad, bias.grad


@pytest.mark.parametrize('d', [128, 768])
@pytest.mark.parametrize('M', [37, 260])
def test_resid_bwd_and_one_segment_ln_resid_bwd(M, d):
    """vlmo_resid_bwd: dz = mask * dx * gamma * row scale / (1 - p), dgamma = sum dx * row scale * zd, dbias = sum dz.
    vlmo_ln_resid_bwd: the same on the dx its LayerNorm backward wrote (dx = LN'(dy) + dres), dx / dw / db against
    autograd too.  Bounds: fp32 outputs and column sums as test_layernorm_fwd_bwd holds them (1e-3 relative + 1e-3,
    sums 1e-3 sqrt(M)).  dz is ONE bf16 rounding of an fp32 product: 2^-8 relative (written 1 / 128 as elsewhere);
    after the LayerNorm backward it and the two sums inherit dx's absolute 1e-3 times the factor dx is multiplied by
    (`amp`, from the inputs alone)."""
    g = torch.Generator().manual_seed(M + d)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    seed = 0x1234567ABCDEF01 + M
    keep = _keep(seed, M, d)
    gamma, bias, pre = r(d), r(d) * 0.1 + 0.3, r(M, d)
    scale = torch.tensor([0.0, 1 / 0.9, 1 / 0.9, 0.0, 1 / 0.9, 1 / 0.9, 1 / 0.9], device=DEV)
    ridx = torch.randint(0, 7, (M,), generator=g).to(torch.int32).to(DEV)
    rows = scale[ridx.long()]
    sq = math.sqrt(M)
    z = lambda *s: torch.zeros(*s, device=DEV)

    dx = r(M, d)
    zd, dpre, dgam, dbias = _branch_reference(pre, bias, gamma, rows, keep, dx)
    dz, dg, db = torch.full((M, d), float('nan'), device=DEV, dtype=torch.bfloat16), z(d), z(d)
    hip.resid_bwd(dx, zd.bfloat16(), gamma, scale, dz, dg, db, M, d, drop=DROP, seed=seed, row_index=ridx)
    for what, got, ref, tol in (('resid_bwd dz', dz, dpre, (1 / 128, 1e-6)), ('resid_bwd dgamma', dg, dgam, (1e-3, 1e-3 * sq)),
                                ('resid_bwd dbias', db, dbias, (1e-3, 1e-3 * sq))):
        _report(what, got, ref)
        _close(got, ref, *tol, what)
    assert torch.equal(dz[rows == 0], torch.zeros_like(dz[rows == 0])), 'a row whose path was dropped has a gradient'

    # fused with the LayerNorm backward above the branch
    x = r(M, d) * 2 + 0.5
    w, b = r(d) * 0.1 + 1, r(d) * 0.1
    dy, dres = r(M, d).bfloat16(), r(M, d)
    mean, rstd = x.mean(1), (x.var(1, unbiased=False) + 1e-12).rsqrt()
    xr, wr, br = (t.double().clone().requires_grad_(True) for t in (x, w, b))
    F.layer_norm(xr, (d,), wr, br, 1e-12).backward(dy.double())
    dx_ref = xr.grad + dres.double()
    zd, dpre, dgam, dbias = _branch_reference(pre, bias, gamma, rows, keep, dx_ref)
    amp_z = max(1.0, gamma.abs().max().item() * rows.max().item() * INV)          # |d dz / d dx|
    amp_g = max(1.0, rows.max().item() * zd.abs().max().item())                   # |d dgamma term / d dx|
    dx1, dw1, db1 = torch.full((M, d), float('nan'), device=DEV), z(d), z(d)
    dz1, dg1, dpb1 = torch.full((M, d), float('nan'), device=DEV, dtype=torch.bfloat16), z(d), z(d)
    hip.ln_resid_bwd(dy, x, w, mean, rstd, dres, dx1, dw1, db1, zd.bfloat16(), gamma, scale, ridx, dz1, dg1, dpb1, M, d,
                     drop=DROP, seed=seed)
    for what, got, ref, tol in (('ln_resid_bwd dx', dx1, dx_ref, (1e-3, 1e-3)), ('ln_resid_bwd dw', dw1, wr.grad, (1e-3, 1e-3 * sq)),
                                ('ln_resid_bwd db', db1, br.grad, (1e-3, 1e-3 * sq)),
                                ('ln_resid_bwd dz', dz1, dpre, (1 / 128, 1e-3 * amp_z)),
                                ('ln_resid_bwd dgamma', dg1, dgam, (1e-3, 1e-3 * sq * amp_g)),
                                ('ln_resid_bwd dbias', dpb1, dbias, (1e-3, 1e-3 * sq * amp_z))):
        _report(what, got, ref)
        _close(got, ref, *tol, what)
    # the mask itself: in the rows whose path is kept, dz is zero exactly where the replica drops it
    _check_mask(dz1[rows != 0], (dx_ref * gamma.double())[rows != 0], keep[rows != 0], 'ln_resid_bwd dz')


# ------------------------------------------------------------------------------------------------ embeddings
@pytest.mark.parametrize('npatch', [4, 196])
def test_embed_img_fwd_bwd(npatch):
    """x = dropout(cls | mask token | proj, + pos) + type row; the mask is indexed (b * (npatch + 1) + t) * d + c"""
    B, d = 3, 128
    seed = 99 + npatch
    keep = _keep(seed, B * (npatch + 1), d).view(B, npatch + 1, d)
    proj = _rand(B * npatch, d, seed=1)
    cls_tok, mask_tok = [_rand(d, seed=s, dtype=torch.float32) for s in (2, 3)]
    pos = _rand(npatch + 1, d, seed=4, dtype=torch.float32)
    type_row = _rand(d, seed=5, dtype=torch.float32)
    g = torch.Generator().manual_seed(npatch)
    masked = (torch.rand(B, npatch, generator=g) < 0.4).to(torch.uint8).to(DEV)
    assert masked.any() and not masked.all()
    x = torch.full((B, npatch + 1, d), float('nan'), device=DEV)
    hip.embed_img_finish(proj, cls_tok, mask_tok, pos, type_row, masked, x, B, npatch, d, drop=DROP, seed=seed)
    pr = proj.double().view(B, npatch, d).clone().requires_grad_(True)
    leaves = [t.double().clone().requires_grad_(True) for t in (cls_tok, mask_tok, pos, type_row)]
    w = masked.double().unsqueeze(-1)
    pre = torch.cat([leaves[0].expand(B, 1, d), pr * (1 - w) + leaves[1] * w], 1) + leaves[2]
    xr = pre * keep * INV + leaves[3]
    # (a): a dropped element is the type row exactly (0 + t); a kept one could only equal it if its value vanished
    # beside the type row's in fp32 -- those are the elements left out
    vanish = (pre.detach() * INV).abs() < 2.0 ** -22 * type_row.double().abs()
    assert int(vanish.sum()) <= CAP * vanish.numel()
    bad = ((x == type_row) != ~keep) & ~vanish
    print(f'embed_img: {int(vanish.sum())} elements left out, {int(bad.sum())} mask mismatches')
    assert not bad.any(), f'embed_img: {int(bad.sum())} elements disagree with the replicated mask, first {bad.nonzero()[0].tolist()}'
    assert int(vanish.sum()) == 0
    _report('embed_img fwd', x, xr.detach())
    _close(x, xr.detach(), 1e-6, 1e-6, 'embed_img fwd')
    dx = _rand(B, npatch + 1, d, seed=6, dtype=torch.float32)
    xr.backward(dx.double())
    dproj = torch.full((B * npatch, d), float('nan'), device=DEV, dtype=torch.bfloat16)
    dcls, dmask, dtype_row = [torch.zeros(d, device=DEV) for _ in range(3)]
    dpos = torch.zeros(npatch + 1, d, device=DEV)
    hip.embed_img_bwd(dx, masked, dproj, dcls, dmask, dpos, dtype_row, B, npatch, d, drop=DROP, seed=seed)
    _close(dproj.view(B, npatch, d), pr.grad, 1 / 128, 1e-3, 'dproj')
    # column sums over the batch and, for the type row and the mask token, over the positions too: 1e-4 relative of
    # test_embed_img_fwd_bwd, the absolute part scaled with the square root of the number of terms (16 positions there)
    many = 1e-4 * max(1.0, math.sqrt((npatch + 1) / 17))
    for got, leaf, name, atol in ((dcls, leaves[0], 'dcls', 1e-4), (dmask, leaves[1], 'dmask', many),
                                  (dpos, leaves[2], 'dpos', 1e-4), (dtype_row, leaves[3], 'dtype', many)):
        _report('embed_img ' + name, got, leaf.grad)
        _close(got, leaf.grad, 1e-4, atol, name)


def _txt_tables(V, T, d):
    return [_rand(V, d, seed=1, dtype=torch.float32), _rand(T, d, seed=2, dtype=torch.float32),
            _rand(d, seed=3, dtype=torch.float32), _rand(d, seed=4, dtype=torch.float32) * 0.1 + 1,
            _rand(d, seed=5, dtype=torch.float32) + 0.5, _rand(d, seed=6, dtype=torch.float32)]


def _txt_reference(tabs, tok, position, keep, dx):
    """rows of tokens `tok` at positions `position`: LayerNorm(word + type0 + pos) -> dropout -> + token type"""
    L = [t.double().clone().requires_grad_(True) for t in tabs]
    e = F.embedding(tok, L[0], padding_idx=0) + L[2] + L[1][position]
    pre = F.layer_norm(e, (e.shape[-1],), L[3], L[4], 1e-12)
    xr = pre * keep * INV + L[5]
    xr.backward(dx.double())
    return pre.detach(), xr.detach(), [leaf.grad for leaf in L]


def _check_txt(what, x, type0, pre, keep, xr, outs, grads):
    vanish = (pre * INV).abs() < 2.0 ** -22 * type0.double().abs()
    bad = ((x == type0) != ~keep) & ~vanish
    print(f'{what}: {int(vanish.sum())} elements left out, {int(bad.sum())} mask mismatches')
    assert int(vanish.sum()) <= CAP * vanish.numel()
    assert not bad.any(), f'{what}: {int(bad.sum())} elements disagree with the replicated mask, first {bad.nonzero()[0].tolist()}'
    assert int(vanish.sum()) == 0
    _report(what + ' fwd', x, xr)
    _close(x, xr, 1e-4, 1e-4, what + ' fwd')
    for got, ref, name in zip(outs, grads, ('dword', 'dpos', 'dbtype0', 'dlnw', 'dlnb', 'dtype0')):
        _report(f'{what} {name}', got, ref)
        _close(got, ref, 1e-3, 1e-3, f'{what} {name}')
    assert torch.equal(outs[0][0], torch.zeros_like(outs[0][0])), 'word row 0 (padding_idx) received a gradient'


def test_embed_txt_fwd_bwd():
    B, T, d, V = 3, 16, 128, 50
    seed = 2 ** 62 - 5
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, V, (B, T), generator=g).to(DEV)
    ids[0, 5:] = 0
    tabs = _txt_tables(V, T, d)
    keep = _keep(seed, B * T, d)
    x = torch.full((B * T, d), float('nan'), device=DEV)
    xhat, rstd = torch.empty(B * T, d, device=DEV), torch.empty(B * T, device=DEV)
    hip.embed_txt_fwd(ids, *tabs, x, xhat, rstd, B, T, d, 1e-12, drop=DROP, seed=seed)
    dx = _rand(B * T, d, seed=7, dtype=torch.float32)
    position = torch.arange(T, device=DEV).repeat(B)
    pre, xr, grads = _txt_reference(tabs, ids.view(-1), position, keep, dx)
    outs = [torch.zeros_like(t) for t in tabs]
    hip.embed_txt_bwd(dx, ids, xhat, rstd, tabs[3], *outs, B, T, d, drop=DROP, seed=seed)
    _check_txt('embed_txt', x, tabs[5], pre, keep, xr, outs, grads)


def test_embed_txt_rows_fwd_bwd_indexes_the_mask_by_packed_row():
    """row-table form, rows of unequal length: packed row m embeds ids[b, t] and takes mask row m -- not row b * T + t"""
    B, T, d, V = 3, 16, 128, 50
    lens = [16, 5, 9]
    seed = 1234
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(1, V, (B, T), generator=g).to(DEV)
    ids[2, 7] = 0                                       # a padding id inside a kept row
    src = torch.tensor([b * T + t for b, n in enumerate(lens) for t in range(n)], dtype=torch.int64, device=DEV)
    off = torch.tensor([sum(lens[:b]) for b in range(B + 1)], dtype=torch.int32, device=DEV)
    nt = sum(lens)
    tabs = _txt_tables(V, T, d)
    keep = _keep(seed, nt, d)
    assert not torch.equal(keep[lens[0]:], _keep(seed, B * T, d)[src[lens[0]:]]), 'the two index spaces give one mask'
    x = torch.full((nt, d), float('nan'), device=DEV)
    xhat, rstd = torch.empty(nt, d, device=DEV), torch.empty(nt, device=DEV)
    hip.embed_txt_rows_fwd(ids, src.to(torch.int32), *tabs, x, xhat, rstd, nt, T, d, 1e-12, drop=DROP, seed=seed)
    dx = _rand(nt, d, seed=8, dtype=torch.float32)
    pre, xr, grads = _txt_reference(tabs, ids.view(-1)[src], src % T, keep, dx)
    outs = [torch.zeros_like(t) for t in tabs]
    hip.embed_txt_rows_bwd(dx, ids, off, xhat, rstd, tabs[3], *outs, B, T, max(lens), d, drop=DROP, seed=seed)
    _check_txt('embed_txt_rows', x, tabs[5], pre, keep, xr, outs, grads)
