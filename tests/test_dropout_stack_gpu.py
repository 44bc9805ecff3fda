"""The block stack in training mode (hidden dropout, attention dropout, drop-path) against the fp64 training-mode
oracle (oracle/vlmo_oracle.py, Train), mask for mask and scale for scale.

Nothing here mirrors an order of RNG draws: the tests call the interfaces that take the randomness as arguments --
Block.meta(..., seed, drop_scales=...) and engine.StackFn.apply(x, metas, *params), exactly as VLMO._run_blocks does,
and VLMO._embed(..., seed) -- with an explicit base seed (block i gets seed + 1000 * (i + 1)) and an explicit
[block, branch, stream, B] tensor of drop-path scales.  The oracle gets the same x, weights and scales, and masks
built on the host from the replicas of the two hashes (tests/dropmask.py, tests/attn_counter.py) with the seed
offsets of csrc/block.hip and the packed-row layout of engine.Plan ("Dropout wiring"):

    proj   seed + 1              rows of the block's whole packed matrix [M, d]
    attn   seed + 11 + launch    sequence index within the forward launch (seg_sep: image sequences, then text)
    fc1    seed + 20 + 2 x       rows of expert x's own range [rows_x, hidden]
    fc2    seed + 21 + 2 x       rows of expert x's own range [rows_x, d]

Bounds: identical masks make the training pass the eval-mode arithmetic with some elements zeroed and the rest scaled
by 1 / 0.9, so they are the ones test_edge_shapes_and_fusion_layer_override_vs_oracle holds at this preset: 3e-2
absolute on the output, 6e-2 of the norm on every gradient (the gradient of the stack's input included).

Sensitivity controls (oracle only, no device): the same oracle run with one wiring error -- a site's mask from the
neighbouring seed offset, the text sequences of the shared attention launch counted from 0, the rows of the second
expert counted from the launch's first row, the drop-path scales of the neighbouring sample -- must differ from the
correct run by more than 3x the bound in the output or in at least one gradient: the comparison above would fail for
each of them."""
from functools import partial

import pytest
import torch

from oracle import synth, vlmo_oracle
from tests import attn_counter, dropmask

DEV = 'cuda'
P_DROP = 0.1
THRESH, INV = dropmask.thresh_of(P_DROP)
OUT_TOL, GRAD_TOL = 3e-2, 6e-2
SEED = 0x5EED1234ABCD

# seed offsets inside a block (csrc/block.hip); a control replaces one entry
# (`only`: in the n-th block of the case alone)
WIRING = dict(proj=1, attn=11, gelu=(20, 22), fc2=(21, 23), txt_seq0=None, expert1_row0=0, roll_scales=0, only=None)


def _mc():
    return synth.make_config('mini').model


def _sd(mc):
    return synth.synth_backbone_state_dict(mc, 0, [('v', 'l', 'vl')] * mc.depth)


class Case:
    """Inputs of one stack case, all on the host: x_t [B, T, d] / x_i [B, P, d] (None when the stream is absent),
    key masks, cotangents, the drop-path scales [block, branch, stream, B] (stream 0 = text, 1 = image)."""

    def __init__(self, name, mode, layers, B, T, P, fusion=0):
        mc = _mc()
        self.name, self.mode, self.layers, self.B, self.T, self.P, self.fusion = name, mode, layers, B, T, P, fusion
        self.d, self.hidden, self.heads = mc.embed_dim, int(mc.embed_dim * mc.mlp_ratio), mc.num_heads
        g = torch.Generator().manual_seed(B * 1000 + T * 10 + P)
        r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()
        self.x_t, self.R_t = (r(B, T, self.d), r(B, T, self.d)) if T else (None, None)
        self.x_i, self.R_i = (r(B, P, self.d), r(B, P, self.d)) if P else (None, None)
        self.tmask = torch.ones(B, T, dtype=torch.int64) if T else None
        self.imask = torch.ones(B, P, dtype=torch.int64) if P else None
        if T:
            self.tmask[-1, T - 3:] = 0                  # last sample padded
        if P:
            self.imask[1, 5:8] = 0                      # a key mask inside an image sequence
        keep = 1.0 - P_DROP
        sc = torch.full((len(layers), 2, 2, B), 1.0 / keep)
        for n in range(len(layers)):
            fused = self.fused(layers[n])
            sc[n, 0, 0, n % B] = 0.0                    # attention branch of one sample dropped, its FFN branch kept
            sc[n, 1, 0, (n + 2) % B] = 0.0
            if fused or not (T and P):                  # one draw per sample: both streams share it
                sc[n, :, 1] = sc[n, :, 0]
            else:                                       # text and image streams of a sample drop independently
                sc[n, 1, 1, n % B] = 0.0
                sc[n, 0, 1, (n + 1) % B] = 0.0
        self.scales = sc

    def fused(self, i):
        return self.mode == 'vl' and i >= self.fusion

    def pack(self, t, i):
        """[B, T, n] / [B, P, n] -> packed rows [M, n]: all text rows (b * T + t), then all image rows"""
        parts = [v.reshape(-1, v.shape[-1]) for v in (t, i) if v is not None]
        return torch.cat(parts)

    def unpack(self, m):
        nt = self.B * self.T
        t = m[:nt].view(self.B, self.T, -1) if self.T else None
        i = m[nt:].view(self.B, self.P, -1) if self.P else None
        return t, i


CASES = {
    'one block, image route': lambda: Case('v', 'v', [0], 3, 0, 17),
    'two blocks, text route': lambda: Case('l', 'l', [0, 1], 3, 9, 0),
    'two blocks, vl, fusion_layer 1': lambda: Case('vl', 'vl', [0, 1], 3, 9, 17, fusion=1),
}


def _trains(case, n, W):
    """{stream: Train} of the n-th block of the case under wiring W: 't' / 'i' below the fusion layer, 'vl' above"""
    i = case.layers[n]
    if W['only'] is not None and W['only'] != n:
        W = WIRING
    B, T, P, d, hid, H = case.B, case.T, case.P, case.d, case.hidden, case.heads
    sb = SEED + 1000 * (i + 1)
    nt, ni = B * T, B * P
    M = nt + ni
    fused = case.fused(i)
    two_experts = case.mode == 'vl' and not fused
    km = lambda off, rows, cols, row0=0: dropmask.keep_mask(sb + off, rows, cols, THRESH, row0)
    proj_t, proj_i = case.unpack(km(W['proj'], M, d))
    if two_experts:
        r0 = W['expert1_row0']
        gelu_t, gelu_i = km(W['gelu'][0], nt, hid).view(B, T, hid), km(W['gelu'][1], ni, hid, r0).view(B, P, hid)
        fc2_t, fc2_i = km(W['fc2'][0], nt, d).view(B, T, d), km(W['fc2'][1], ni, d, r0).view(B, P, d)
    else:
        gelu_t, gelu_i = case.unpack(km(W['gelu'][0], M, hid))
        fc2_t, fc2_i = case.unpack(km(W['fc2'][0], M, d))
    sc = case.scales[n].double()
    if W['roll_scales']:
        sc = sc.roll(W['roll_scales'], dims=-1)
    aseed = sb + W['attn']
    if fused:
        attn = attn_counter.keep_mask(aseed, [T + P] * B, H, THRESH)
        cat = lambda a, b: torch.cat([a, b], 1)
        return {'vl': vlmo_oracle.Train(attn, cat(proj_t, proj_i), cat(gelu_t, gelu_i), cat(fc2_t, fc2_i), INV, sc[0, 0], sc[1, 0])}
    out = {}
    if P:       # image sequences come first in the shared launch
        out['i'] = vlmo_oracle.Train(attn_counter.keep_mask(aseed, [P] * B, H, THRESH), proj_i, gelu_i, fc2_i, INV, sc[0, 1], sc[1, 1])
    if T:
        seq0 = (B if P else 0) if W['txt_seq0'] is None else W['txt_seq0']
        out['t'] = vlmo_oracle.Train(attn_counter.keep_mask(aseed, [T] * B, H, THRESH, seq0=seq0), proj_t, gelu_t, fc2_t, INV,
                                     sc[0, 0], sc[1, 0])
    return out


def _oracle(case, W=WIRING):
    """packed output [M, d], {parameter name: gradient} and the packed input gradient of the case under wiring W"""
    mc = _mc()
    sd = {k: v.double().requires_grad_(True) for k, v in _sd(mc).items()}
    xt = case.x_t.clone().requires_grad_(True) if case.T else None
    xi = case.x_i.clone().requires_grad_(True) if case.P else None
    t, im, x = xt, xi, None
    for n, i in enumerate(case.layers):
        tr = _trains(case, n, W)
        if case.fused(i):
            if x is None:
                x = torch.cat([t, im], 1)               # text first
            x = vlmo_oracle.block(sd, i, x, torch.cat([case.tmask, case.imask], 1), 'vl', case.heads, tr['vl'])
        else:
            if t is not None:
                t = vlmo_oracle.block(sd, i, t, case.tmask, 'l', case.heads, tr['t'])
            if im is not None:
                im = vlmo_oracle.block(sd, i, im, case.imask, 'v', case.heads, tr['i'])
    if x is not None:
        t, im = x[:, :case.T], x[:, case.T:]
    out = case.pack(t, im)
    (out * case.pack(case.R_t, case.R_i)).sum().backward()
    grads = {k: v.grad for k, v in sd.items() if v.grad is not None and v.grad.abs().max() > 0}
    dx = case.pack(xt.grad if xt is not None else None, xi.grad if xi is not None else None)
    return out.detach(), grads, dx


_ORACLE = {}


def _oracle_of(key):
    """the correct oracle run of a case: computed once, shared by the control and the GPU comparison, never written"""
    if key not in _ORACLE:
        case = CASES[key]()
        _ORACLE[key] = (case,) + _oracle(case)
    return _ORACLE[key]


def _controls(case):
    c = {'proj mask from seed + 2': dict(proj=2), 'attention mask from seed + 12': dict(attn=12),
         'fc1 mask from seed + 21': dict(gelu=(21, 23)), 'fc2 mask from seed + 20': dict(fc2=(20, 22)),
         'drop-path scales of the neighbouring sample': dict(roll_scales=1)}
    if len(case.layers) > 1:      # the block whose FFN branch the backward of the block above regenerates
        c['fc2 mask of the lower block alone from seed + 20'] = dict(fc2=(20, 22), only=0)
        c['drop-path scales of the lower block alone, neighbouring sample'] = dict(roll_scales=1, only=0)
    if case.mode == 'vl':
        c['text sequences of the shared launch counted from attn_seq0 = 0'] = dict(txt_seq0=0)
        c['image expert rows counted from the launch (row0 = nt)'] = dict(expert1_row0=case.B * case.T)
        c['image expert under the text expert\'s seeds'] = dict(gelu=(20, 20), fc2=(21, 21))
    return c


@pytest.mark.parametrize('key', list(CASES))
def test_oracle_controls_each_wiring_error_exceeds_three_times_the_bound(key):
    """CPU only.  No case needed a larger cotangent or rate.  Every control reaches 3x in a gradient (the output alone
    would not do: a wrong attention mask moves it by 0.8 - 1.0x the bound); the weakest of each case: image route,
    attention mask from seed + 12: 7.2x (proj.weight); text route, proj mask from seed + 2: 7.9x (q_bias); vl, text
    sequences counted from attn_seq0 = 0: 5.6x (blocks.0.attn.qkv.weight); the others 7.7 - 20x."""
    case, out, grads, dx = _oracle_of(key)
    rate = 1 - torch.cat([t.gelu.reshape(-1) for t in _trains(case, 0, WIRING).values()]).float().mean().item()
    assert abs(rate - P_DROP) < 0.01, rate
    for what, change in _controls(case).items():
        o2, g2, dx2 = _oracle(case, {**WIRING, **change})
        out_ratio = (o2 - out).abs().max().item() / OUT_TOL
        rel = {k: (g2[k] - grads[k]).norm().item() / grads[k].norm().item() for k in grads}
        rel['input'] = (dx2 - dx).norm().item() / dx.norm().item()
        k = max(rel, key=rel.get)
        print(f'{case.name}: {what}: output {out_ratio:.1f}x the bound, gradient of {k} {rel[k] / GRAD_TOL:.1f}x the bound')
        assert out_ratio > 3 or rel[k] / GRAD_TOL > 3, (what, out_ratio, rel[k] / GRAD_TOL)


def _model(mc):
    from exploremultimodal_amd.vlmo import VLMO, LayerNorm
    m = VLMO(img_size=mc.img_size, patch_size=mc.patch_size, in_chans=mc.in_chans, num_classes=mc.num_classes,
             embed_dim=mc.embed_dim, depth=mc.depth, num_heads=mc.num_heads, mlp_ratio=mc.mlp_ratio,
             qkv_bias=mc.qkv_bias, drop_rate=P_DROP, attn_drop_rate=P_DROP, drop_path_rate=P_DROP,
             norm_layer=partial(LayerNorm, eps=1e-12), init_values=mc.init_values, vocab_size=mc.vocab_size,
             max_text_len=mc.max_text_len, fusion_layer=mc.fusion_layer)
    m.load_state_dict(_sd(mc), strict=True)
    for blk in m.blocks:            # linspace(0, rate, depth) gives block 0 no drop-path: every block takes its scales here
        blk.drop_path_rate = P_DROP
    return m.to(DEV).train()


def _compare_grads(named, grads, what):
    worst = (0.0, '')
    for k, p in named:
        ref = grads.get(k)
        if ref is None:
            assert p.grad is None or p.grad.abs().max().item() <= 1e-6, f'{what}: {k} has a gradient the oracle has not'
            continue
        assert p.grad is not None, f'{what}: {k} has no gradient'
        rel = (p.grad.detach().cpu().double() - ref).norm().item() / ref.norm().item()
        worst = max(worst, (rel, k))
        assert rel <= GRAD_TOL, f'{what}: gradient of {k} off by {rel:.4f} of its norm (bound {GRAD_TOL})'
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize('key', list(CASES))
def test_stack_matches_the_training_mode_oracle(key):
    """Measured on an MI355X (max |stack - oracle| against 3e-2; worst parameter gradient and the input gradient
    against 6e-2 of their norm): image route 7.1e-4, blocks.0.attn.q_bias 5.2e-3, 1.2e-4; text route 6.2e-4, q_bias
    5.2e-3, 1.7e-4; vl 7.7e-4, q_bias 6.9e-3, 1.7e-4 -- no bound needed the 1 / 0.9 factor.  With seed1 of the
    two-segment norm1 backward deliberately set to the text expert's (seed + 21) the vl case, and only it, failed with
    blocks.0.norm2.weight off by 0.36 of its norm."""
    from exploremultimodal_amd import engine
    case, out, grads, dx = _oracle_of(key)
    mc = _mc()
    model = _model(mc)
    B, T, P = case.B, case.T, case.P
    plan = engine.Plan(B, T, P, DEV, case.tmask.to(DEV) if T else None, case.imask.to(DEV) if P else None)
    # the hand-written layout of Case.pack is engine.Plan's: packed row -> row of the [B, T + P, d] output
    rows = torch.arange(B * (T + P)).view(B, T + P, 1)
    assert torch.equal(case.pack(rows[:, :T] if T else None, rows[:, T:] if P else None).view(-1), plan.rowmap.cpu().long())
    x = case.pack(case.x_t, case.x_i).float().to(DEV).requires_grad_(True)
    scales = case.scales.to(DEV)
    metas, params = [], []
    for n, i in enumerate(case.layers):
        routes, ranges, fused = model._routes(i, case.mode, case.fusion, plan)
        assert fused == case.fused(i)
        mt, ps = model.blocks[i].meta(x, plan, routes, ranges, fused, model._shadows, SEED + 1000 * (i + 1),
                                      drop_scales=scales[n])
        assert mt.rs1 is not None and mt.drop[0] == THRESH and mt.attn_drop[0] == THRESH
        metas.append(mt)
        params += ps
    y = engine.StackFn.apply(x, metas, *params)
    (y * case.pack(case.R_t, case.R_i).float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    err = (y.detach().cpu().double() - out).abs().max().item()
    print(f'{case.name}: max |stack - oracle| = {err:.4g} (bound {OUT_TOL})')
    rel_dx = (x.grad.cpu().double() - dx).norm().item() / dx.norm().item()
    print(f'{case.name}: input gradient off by {rel_dx:.4g} of its norm (bound {GRAD_TOL})')
    named = [(k, p) for k, p in model.named_parameters() if k.startswith('blocks.')]
    assert {k for k in grads} <= {k for k, _ in named}
    worst = _compare_grads(named, grads, case.name)
    print(f'{case.name}: worst parameter gradient {worst[1]} off by {worst[0]:.4g} of its norm (bound {GRAD_TOL}), '
          f'{len(grads)} gradients compared')
    assert err <= OUT_TOL, (case.name, err)
    assert rel_dx <= GRAD_TOL, (case.name, rel_dx)


# ------------------------------------------------------------------------------------------------ embedding dropout
def _embed_inputs(mc, B, T):
    g = torch.Generator().manual_seed(17)
    img = torch.randn(B, mc.in_chans, mc.img_size, mc.img_size, generator=g)
    ids = torch.randint(1, mc.vocab_size, (B, T), generator=g)
    ids[-1, T - 3:] = 0
    npatch = synth.num_img_tokens(mc) - 1
    bmp = torch.rand(B, npatch, generator=g) < 0.4
    return img, ids, bmp


def _embed_oracle(mc, mode, B, T, seeds=(1, 2)):
    """packed output and gradients of the embeddings under an explicit seed: text mask from seed + seeds[0] over the
    packed text rows [B T, d], image mask from seed + seeds[1] over (b * P + t) * d + c"""
    sd = {k: v.double().requires_grad_(True) for k, v in _sd(mc).items()}
    img, ids, bmp = _embed_inputs(mc, B, T)
    P, d = synth.num_img_tokens(mc), mc.embed_dim
    parts = []
    if mode in ('l', 'vl'):
        keep = dropmask.keep_mask(SEED + seeds[0], B * T, d, THRESH).view(B, T, d)
        parts.append(vlmo_oracle.embed_txt(sd, mc, ids, keep=keep, inv_keep=INV).reshape(-1, d))
    if mode in ('v', 'vl'):
        keep = dropmask.keep_mask(SEED + seeds[1], B * P, d, THRESH).view(B, P, d)
        parts.append(vlmo_oracle.embed_img(sd, mc, img.double(), bmp, keep=keep, inv_keep=INV).reshape(-1, d))
    out = torch.cat(parts)
    R = torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    (out * R).sum().backward()
    return out.detach(), {k: v.grad for k, v in sd.items() if v.grad is not None and v.grad.abs().max() > 0}, R


@pytest.mark.parametrize('mode', ['v', 'l', 'vl'])
def test_oracle_control_embedding_masks_under_each_other_s_seed(mode):
    mc = _mc()
    out, grads, _ = _embed_oracle(mc, mode, 3, 9)
    o2, g2, _ = _embed_oracle(mc, mode, 3, 9, seeds=(2, 1))
    ratio = (o2 - out).abs().max().item() / OUT_TOL
    print(f'embedding {mode}: seeds swapped: output {ratio:.1f}x the bound')
    assert ratio > 3


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['v', 'l', 'vl'])
def test_embedding_dropout_matches_the_oracle(mode):
    """VLMO._embed with an explicit seed: the text embedding drops under seed + 1, the image embedding under seed + 2,
    each over its own packed rows."""
    from exploremultimodal_amd import engine
    mc = _mc()
    B, T = 3, 9
    P = synth.num_img_tokens(mc)
    out, grads, R = _embed_oracle(mc, mode, B, T)
    model = _model(mc)
    img, ids, bmp = _embed_inputs(mc, B, T)
    plan = engine.Plan(B, T if mode != 'v' else 0, P if mode != 'l' else 0, DEV)
    x = model._embed(plan, img.to(DEV) if mode != 'l' else None, ids.to(DEV) if mode != 'v' else None,
                     bmp.to(DEV) if mode != 'l' else None, 1, SEED)
    (x * R.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    got = x.detach().cpu().double()
    # (a) the mask itself: the oracle's dropped elements are the token-type row exactly, and so are the engine's
    type_rows = model.token_type_embeddings.weight.detach().cpu().double()
    nt = plan.nt
    trow = torch.cat([type_rows[0].expand(nt, -1), type_rows[1].expand(plan.ni, -1)])
    assert torch.equal(got == trow.float().double(), out == trow), 'the engine drops other elements than the replicated mask'
    err = (got - out).abs().max().item()
    print(f'embedding {mode}: max |engine - oracle| = {err:.4g} (bound {OUT_TOL})')
    named = [(k, p) for k, p in model.named_parameters() if not k.startswith('blocks.')]
    worst = _compare_grads(named, grads, f'embedding {mode}')
    print(f'embedding {mode}: worst gradient {worst[1]} off by {worst[0]:.4g} of its norm (bound {GRAD_TOL})')
    assert err <= OUT_TOL, err
