"""The embedding kernels of csrc/elementwise.hip -- patchify, embed_img_finish / embed_img_bwd, embed_txt_fwd / embed_txt_bwd,
the row-table pair embed_txt_rows_fwd / embed_txt_rows_bwd with embed_txt_fold, cast_weight / cast_weight_multi -- at
the widths and launch regimes training runs, against fp64.  Cases, references, units and figures come from
tests/embed_cases.py; tests/test_embedding_cases_cpu.py checks their premises on the CPU.

EXACT cases (integer data, torch.equal with the fp64 result) reach: VPL 1, 2, 3 and 4 of the text kernels and a
partially filled last vector group (d = 300, 772); rows_per_block 4, 8 and 16 with a short last chunk (B = 5, 21, 70)
and B < 4 (waves without a row); masked = None and every optional output passed as null once; non-zero prefill under
every accumulating output; the grid cap of patchify (4100 x 4100) and -- as bit-for-bit agreement of the rows of the
second trip with a one-trip launch of the same rows -- the grid caps of embed_txt_fwd and embed_txt_rows_fwd (32 772
rows); every alignment path of cast_weight / cast_weight_multi.  BOUNDED cases (gaussian data) hold column sums to
(N - 1 + k) u sum|t_i| and per-row results to four times the fp32 emulation's figure; each prints its ratio.

Every output lies inside a NaN-filled allocation with spare elements before and after it (and spare position rows
behind dpos): a store outside the output, or an output element never stored, is seen."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from exploremultimodal_amd import hip  # noqa: E402
from tests import dropmask  # noqa: E402
from tests import embed_cases as ec  # noqa: E402

DEV = 'cuda'
NAN = float('nan')
PAD = 64                                  # spare elements on each side (a multiple of 16 bytes in every type used)
TXT_OUTS = ('dword', 'dpos', 'dbtype0', 'dln_w', 'dln_b', 'dtype0')
SPARE_POS_ROWS = 3


class Guarded:
    """a contiguous tensor `t` of `shape` in the middle of a NaN-filled allocation"""

    def __init__(self, shape, dtype=torch.float32, fill=None):
        self.n = int(math.prod(shape))
        self.buf = torch.full((self.n + 2 * PAD,), NAN, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + self.n].view(shape)
        if fill is not None:
            self.t.copy_(fill)

    def intact(self, what):
        assert self.buf[:PAD].isnan().all() and self.buf[PAD + self.n:].isnan().all(), f'{what}: a store outside the output'


def _prefill(shape, salt):
    """embed_cases.prefill on the device"""
    n = int(math.prod(shape))
    return ((torch.arange(n, dtype=torch.int64, device=DEV) * 7 + salt) % 11 - 5).float().view(shape)


def _dev(t):
    return None if t is None else t.to(DEV)


def _same(got, want64, what):
    """bit-for-bit: the fp32 / bf16 result, widened, is the fp64 one"""
    if not torch.equal(got.double(), want64):
        bad = got.double() != want64
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())}/{bad.numel()} elements differ from the exact result, first at {idx}: '
                             f'got {got[tuple(idx)].item()!r} want {want64[tuple(idx)].item()!r}')


def _ratio(what, got, ref, bound):
    """largest |got - ref| / bound (0 / 0 counts as 0; a NaN or an error where the bound is 0 as infinite)"""
    err = (got.double() - ref).abs()
    r = torch.where(err <= bound, err / bound.clamp_min(1e-300), torch.full_like(err, float('inf')))
    r = torch.where((err == 0) & (bound == 0), torch.zeros_like(r), r).max().item()
    print(f'{what}: max |got - ref| / bound = {r:.4f}')
    assert r <= 1.0, f'{what}: outside the bound ({int((~(err <= bound)).sum())}/{err.numel()} elements, max error {err.max().item():.4g})'
    return r


# ================================================================================================ exact: text backward
def _txt_bwd(c, form, null=()):
    """run one form of the text backward on non-zero prefill; returns {name: Guarded}"""
    B, T, d, V = c['B'], c['T'], c['d'], c['V']
    shapes = {'dword': (V, d), 'dpos': (T + SPARE_POS_ROWS, d), 'dbtype0': (d,), 'dln_w': (d,), 'dln_b': (d,), 'dtype0': (d,)}
    outs = {n: Guarded(s, fill=_prefill(s, i + 1)) for i, (n, s) in enumerate(shapes.items())}
    args = [None if n in null else (outs[n].t[:T] if n == 'dpos' else outs[n].t) for n in TXT_OUTS]
    dx, xhat, rstd, ln_w, ids = (_dev(c[k]) for k in ('dx', 'xhat', 'rstd', 'ln_w', 'ids'))
    if form == 'fixed':
        hip.embed_txt_bwd(dx, ids, xhat, rstd, ln_w, *args, B, T, d, drop=c['drop'], seed=c['seed'])
    else:
        hip.embed_txt_rows_bwd(dx, ids, _dev(c['off']), xhat, rstd, ln_w, *args, B, T, c['maxlen'], d, drop=c['drop'], seed=c['seed'])
    return outs


def _txt_bwd_is_exact(c, outs, what, null=()):
    T = c['T']
    for i, name in enumerate(TXT_OUTS):
        want = _prefill(outs[name].t.shape, i + 1).double()
        if name not in null:
            s = _dev(c['sums'][name])
            if name == 'dword':
                want[_dev(c['sums']['word_ids'])] += s
            elif name == 'dpos':
                want[:T] += s
            else:
                want += s
        _same(outs[name].t, want, f'{what} {name}' + (' (passed as null)' if name in null else ''))
        outs[name].intact(f'{what} {name}')
    assert torch.equal(outs['dword'].t[0], _prefill(outs['dword'].t.shape, 1)[0]), f'{what}: word row 0 (padding_idx) was written'
    assert torch.equal(outs['dpos'].t[T:], _prefill(outs['dpos'].t.shape, 2)[T:]), f'{what}: a position row >= T was written'


@pytest.mark.parametrize('case', ec.TXT_EXACT, ids=ec.txt_exact_id)
def test_txt_bwd_exact(case):
    """embed_txt_bwd and embed_txt_rows_bwd (+ embed_txt_fold) on integer rows: all six gradients equal the fp64 sums
    added onto non-zero prefill, bit for bit -- and therefore each other; word row 0 and the position rows >= T keep
    their prefill.  The id names what the case reaches: VPL, a partial last vector group, rows_per_block, a short last
    chunk, B < 4; ids repeat heavily (one id on >= 64 rows), hold padding id 0 inside the texts, and at V = 40 000
    reach id * d > 2^24.  Then the row-table form on ragged lengths that include 1 and T."""
    c = ec.txt_exact(*case)
    fixed = _txt_bwd(c, 'fixed')
    _txt_bwd_is_exact(c, fixed, 'fixed-length form')
    rows = _txt_bwd(c, 'rows')
    _txt_bwd_is_exact(c, rows, 'row-table form, full lengths')
    for name in TXT_OUTS:
        assert torch.equal(fixed[name].t, rows[name].t), name
    del fixed, rows
    cr = ec.txt_exact(*case, ragged=True)
    _txt_bwd_is_exact(cr, _txt_bwd(cr, 'rows'), f'row-table form, lengths {cr["lens"][:6]}...')


@pytest.mark.parametrize('form', ['fixed', 'rows'])
@pytest.mark.parametrize('null', TXT_OUTS)
def test_txt_bwd_exact_with_a_null_output(null, form):
    """each of the six outputs passed as null once: the other five are still exact, nothing else is written"""
    c = ec.txt_exact(5, 7, 300, True, 50, ragged=form == 'rows')
    _txt_bwd_is_exact(c, _txt_bwd(c, form, null=(null,)), f'{form}, {null} = null', null=(null,))


# ================================================================================================ exact: image
def _img_args(c):
    return [_dev(c[k]) for k in ('cls_tok', 'mask_tok', 'pos', 'type_row', 'masked')]


@pytest.mark.parametrize('case', ec.IMG_EXACT, ids=ec.img_exact_id)
def test_img_fwd_bwd_exact(case):
    """embed_img_finish: x == ((src + pos) keep 2) + type exactly.  embed_img_bwd: dproj == bf16(g) at unmasked patches
    and 0 at masked ones; dcls, dmask, dpos, dtype_row equal the fp64 sums added onto non-zero prefill; each of the four
    passed as null once; with masked = None dmask keeps its prefill.  Cases: mask ratio 0, 1, mixed, masked = None;
    dropout off and p = 0.5."""
    c = ec.img_exact(*case)
    B, npatch, d = c['B'], c['npatch'], c['d']
    proj = _dev(c['proj']).bfloat16()
    cls_tok, mask_tok, pos, type_row, masked = _img_args(c)
    x = Guarded((B, npatch + 1, d))
    hip.embed_img_finish(proj, cls_tok, mask_tok, pos, type_row, masked, x.t, B, npatch, d, drop=c['drop'], seed=c['seed'])
    _same(x.t, _dev(c['x']), 'x')
    x.intact('x')
    dx = _dev(c['dx'])
    shapes = {'dcls': (d,), 'dmask': (d,), 'dpos': (npatch + 1, d), 'dtype_row': (d,)}
    for null in (None,) + ec.IMG_OPTIONAL:
        dproj = Guarded((B * npatch, d), dtype=torch.bfloat16)
        outs = {n: Guarded(s, fill=_prefill(s, i + 1)) for i, (n, s) in enumerate(shapes.items())}
        hip.embed_img_bwd(dx, masked, dproj.t, *[None if n == null else outs[n].t for n in ec.IMG_OPTIONAL], B, npatch, d,
                          drop=c['drop'], seed=c['seed'])
        _same(dproj.t.view(B, npatch, d), _dev(c['sums']['dproj']), f'dproj ({null} = null)')
        dproj.intact('dproj')
        for i, n in enumerate(ec.IMG_OPTIONAL):
            want = _prefill(shapes[n], i + 1).double()
            if n != null and not (n == 'dmask' and masked is None):
                want += _dev(c['sums'][n])
            _same(outs[n].t, want, f'{n} ({null} = null)')
            outs[n].intact(n)


# ================================================================================================ exact: patchify, cast
@pytest.mark.parametrize('shape', ec.PATCHIFY, ids=lambda s: 'x'.join(map(str, s[:4])) + f'-p{s[4]}')
def test_patchify_exact(shape):
    """out == bf16(unfold) at patch 4 / 16 / 32, C = 1 / 3, H != W, the 384 px grid, and 1 x 1 x 4100 x 4100 with patch
    4: 4 202 500 groups of four, beyond the 16 384 workgroups of one trip (the grid-stride loop)"""
    B, C, H, W, p = shape
    img = torch.randn(B, C, H, W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(H + p))
    out = Guarded((B * (H // p) * (W // p), C * p * p), dtype=torch.bfloat16)
    hip.patchify(img, out.t, p)
    assert torch.equal(out.t, ec.patchify_ref(img, p).bfloat16())
    out.intact('patchify')


def _cast_outputs(rows, cols, mode, dtype):
    dst = Guarded((rows, cols), dtype=dtype) if mode in ('dst', 'both') else None
    dstT = Guarded((cols, rows), dtype=dtype) if mode in ('dstT', 'both') else None
    return dst, dstT


def _cast_is_exact(src, dst, dstT, what):
    if dst is not None:
        _same(dst.t, src.double(), f'{what} dst')
        dst.intact(f'{what} dst')
    if dstT is not None:
        _same(dstT.t, src.double().t(), f'{what} dstT')
        dstT.intact(f'{what} dstT')


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_cast_weight_exact_on_every_alignment(dtype):
    """cast_weight and cast_weight_multi (more than the 72 jobs of one launch): rows and cols each a multiple of 64, of
    4 only, or odd; dst only, dstT only, both; values exact in both types, the spare area stays NaN"""
    jobs, held = [], []
    for rep in range(3):
        for rows, cols in ec.CAST_SHAPES:
            src = _dev(ec.cast_src(rows, cols))
            for mode in ec.CAST_MODES:
                if rep == 0:
                    dst, dstT = _cast_outputs(rows, cols, mode, dtype)
                    hip.cast_weight(src, None if dst is None else dst.t, None if dstT is None else dstT.t)
                    _cast_is_exact(src, dst, dstT, f'cast_weight {rows}x{cols} {mode}')
                dst, dstT = _cast_outputs(rows, cols, mode, dtype)
                jobs.append((src, None if dst is None else dst.t, None if dstT is None else dstT.t))
                held.append((src, dst, dstT, f'cast_weight_multi job {len(jobs) - 1}: {rows}x{cols} {mode}'))
    assert len(jobs) > 72
    hip.cast_weight_multi(jobs)
    for h in held:
        _cast_is_exact(*h)


# ================================================================================================ bounded: text
def _mask_positions(what, x, type0, pre, keep, inv):
    """x is the type row exactly where the replicated mask drops, and nowhere else"""
    out = ec.left_out(pre, inv, type0)
    n = int(out.sum())
    bad = ((x == type0) != ~keep) & ~out
    print(f'{what}: {n} elements left out of the mask comparison, {int(bad.sum())} mismatches')
    assert n <= ec.LEFT_OUT_CAP * out.numel() and n == 0
    assert not bad.any(), f'{what}: {int(bad.sum())} elements disagree with the replicated mask, first {bad.nonzero()[0].tolist()}'


def _txt_fwd_bounded(what, tabs, x, xhat, rstd, tok, pos_t, keep, inv):
    e, xhat_r, rstd_r, pre = ec.txt_fwd_ref(tabs, tok, pos_t)
    x_r = pre * (1.0 if keep is None else keep.double() * inv) + tabs[5].double()
    if keep is not None:
        _mask_positions(what, x, tabs[5], pre, keep, inv)
    _ratio(f'{what} x', x, x_r, ec.MARGIN * ec.FIG['x'] * ec.unit_x(x_r, xhat_r, tabs[3], tabs[4]))
    _ratio(f'{what} xhat', xhat, xhat_r, ec.MARGIN * ec.FIG['xhat'] * ec.unit_xhat(xhat_r))
    _ratio(f'{what} rstd', rstd, rstd_r, ec.MARGIN * ec.FIG['rstd'] * ec.unit_rstd(rstd_r))
    return xhat_r.float(), rstd_r.float()


def _txt_bounded(c, lens):
    """forward against fp64, then the backward fed the TRUE xhat / rstd (fp64 rounded to fp32) against the fp64
    restatement on those inputs; lens = None is the fixed-length form, otherwise the row-table form"""
    B, T, d, V = c['B'], c['T'], c['d'], c['V']
    tabs = [_dev(t) for t in c['tabs']]
    ids = _dev(c['ids'])
    if lens is None:
        M, keep = c['M'], _dev(c['keep'])
        src = torch.arange(M, device=DEV)
    else:
        src = torch.tensor([b * T + t for b, n in enumerate(lens) for t in range(n)], device=DEV)
        off = torch.tensor([sum(lens[:b]) for b in range(B + 1)], dtype=torch.int32, device=DEV)
        M = len(src)
        keep = _dev(dropmask.keep_mask(c['seed'], M, d, c['drop'][0])) if c['drop'][0] else None
    tok, pos_t, dx, inv = ids.view(-1)[src], src % T, _dev(c['dx'])[:M].contiguous(), c['drop'][1]
    x, xhat, rstd = Guarded((M, d)), Guarded((M, d)), Guarded((M,))
    if lens is None:
        hip.embed_txt_fwd(ids, *tabs, x.t, xhat.t, rstd.t, B, T, d, ec.EPS, drop=c['drop'], seed=c['seed'])
    else:
        hip.embed_txt_rows_fwd(ids, src.to(torch.int32), *tabs, x.t, xhat.t, rstd.t, M, T, d, ec.EPS, drop=c['drop'], seed=c['seed'])
    xh32, rs32 = _txt_fwd_bounded('fwd', tabs, x.t, xhat.t, rstd.t, tok, pos_t, keep, inv)
    for g in (x, xhat, rstd):
        g.intact('fwd')
    shapes = {'dword': (V, d), 'dpos': (T + SPARE_POS_ROWS, d), 'dbtype0': (d,), 'dln_w': (d,), 'dln_b': (d,), 'dtype0': (d,)}
    outs = {n: Guarded(s, fill=torch.zeros(s, device=DEV)) for n, s in shapes.items()}
    args = [outs[n].t[:T] if n == 'dpos' else outs[n].t for n in TXT_OUTS]
    if lens is None:
        hip.embed_txt_bwd(dx, ids, xh32, rs32, tabs[3], *args, B, T, d, drop=c['drop'], seed=c['seed'])
    else:
        hip.embed_txt_rows_bwd(dx, ids, off, xh32, rs32, tabs[3], *args, B, T, max(lens), d, drop=c['drop'], seed=c['seed'])
    sums, abs_sums, de = ec.txt_bwd_sums(dx, keep, inv, xh32, rs32, tabs[3], tok, pos_t, T)
    for name in ('dtype0', 'dln_b', 'dln_w'):
        _ratio(f'bwd {name}', outs[name].t, sums[name], ec.colsum_bound(name, M, abs_sums[name]))
    # sums of de: each term carries its per-row bound, the N - 1 additions (N - 1) u sum|de|
    gy = dx.double() * (1.0 if keep is None else keep.double() * inv)
    row_bound = ec.MARGIN * ec.FIG['de'] * ec.unit_de(gy * tabs[3].double(), xh32.double(), rs32.double())
    terms = ec.fold_rows(row_bound, tok, pos_t, T)
    count = ec.fold_rows(torch.ones_like(de), tok, pos_t, T)
    for name in ('dbtype0', 'dpos', 'dword'):
        bound = (count[name] - 1).clamp_min(0) * ec.U * abs_sums[name] + terms[name]
        ref = sums[name]
        if name == 'dword':                             # every other word row, row 0 among them, stays exactly zero
            full = torch.zeros(V, d, dtype=torch.float64, device=DEV)
            ref, bound = full.index_copy(0, sums['word_ids'], ref), full.index_copy(0, sums['word_ids'], bound)
        got = outs[name].t[:T] if name == 'dpos' else outs[name].t
        _ratio(f'bwd {name}', got, ref, bound)
    assert torch.equal(outs['dpos'].t[T:], torch.zeros_like(outs['dpos'].t[T:])), 'a position row >= T was written'
    for n in TXT_OUTS:
        outs[n].intact(n)


@pytest.mark.parametrize('case', ec.BOUNDED_TXT, ids=ec.bounded_id)
def test_txt_fwd_bwd_bounded(case):
    """embed_txt_fwd and embed_txt_bwd on gaussian tables at d = 128 ... 1024, B = 5 and 70, dropout off and p = 0.1
    (mask position for position against tests/dropmask.py)"""
    _txt_bounded(ec.txt_bounded(*case), None)


@pytest.mark.parametrize('case', [(5, 16, 300, True), (70, 16, 768, True), (70, 16, 772, False)], ids=ec.bounded_id)
def test_txt_rows_fwd_bwd_bounded(case):
    """the row-table pair on ragged lengths, the mask indexed by the packed row"""
    c = ec.txt_bounded(*case)
    _txt_bounded(c, ec.ragged_lens(c['B'], c['T'], torch.Generator().manual_seed(c['B'])))


@pytest.mark.parametrize('form', ['fixed', 'rows'])
def test_txt_fwd_grid_cap(form):
    """32 772 rows at d = 64: more than the 8192 workgroups x 4 rows of one trip, so embed_txt_fwd / embed_txt_rows_fwd
    take the grid-stride loop.  With p = 0.1: all rows within the bounds, the mask position for position.  Without
    dropout: the rows of the second trip equal, bit for bit, a one-trip launch of the same rows."""
    B, T, d = ec.TXT_CAP
    ntok = B * T
    c, src, keep = ec.txt_cap_case(form)                    # rows: 32 772 of 33 600 positions, in order
    tabs, ids, src, keep = [_dev(t) for t in c['tabs']], _dev(c['ids']), _dev(src), _dev(keep)
    src32 = src.to(torch.int32)
    tok, pos_t = ids.view(-1)[src], src % T

    def run(drop, rows=None):
        """the whole case, or the packed rows `rows` of it alone"""
        n = ntok if rows is None else len(rows)
        x, xhat, rstd = Guarded((n, d)), Guarded((n, d)), Guarded((n,))
        if form == 'rows':
            hip.embed_txt_rows_fwd(ids, src32 if rows is None else src32[rows].contiguous(), *tabs, x.t, xhat.t, rstd.t, n, T, d,
                                   ec.EPS, drop=drop, seed=c['seed'])
        elif rows is None:
            hip.embed_txt_fwd(ids, *tabs, x.t, xhat.t, rstd.t, B, T, d, ec.EPS, drop=drop, seed=c['seed'])
        else:                                               # the last sample alone
            hip.embed_txt_fwd(ids[B - 1:].contiguous(), *tabs, x.t, xhat.t, rstd.t, 1, T, d, ec.EPS, drop=drop, seed=c['seed'])
        for g in (x, xhat, rstd):
            g.intact('grid cap')
        return x.t, xhat.t, rstd.t

    x, xhat, rstd = run(c['drop'])
    _txt_fwd_bounded(f'{form}, 32 772 rows', tabs, x, xhat, rstd, tok, pos_t, keep, c['drop'][1])
    whole = run((0, 1.0))
    last = torch.arange(ntok - T, ntok, device=DEV)         # rows 32 760 .. 32 771: the last four are in the second trip
    assert ntok - 4 >= 4 * ec.TXT_FWD_GRID_CAP
    for a, b, name in zip(whole, run((0, 1.0), rows=last), ('x', 'xhat', 'rstd')):
        assert torch.equal(a[ntok - T:], b), f'{name}: the rows of the second trip differ from a one-trip launch'


# ================================================================================================ bounded: image
@pytest.mark.parametrize('case', ec.BOUNDED_IMG, ids=lambda c: f'B{c[0]}-np{c[1]}-d{c[2]}-{"p0.1" if c[3] else "nodrop"}')
def test_img_fwd_bwd_bounded(case):
    """gaussian data: x within its four roundings, dproj within two fp32 roundings and the bf16 one, the four vectors within
    (N - 1 + k) u sum|t_i|"""
    c = ec.img_bounded(*case)
    B, npatch, d, inv = c['B'], c['npatch'], c['d'], c['drop'][1]
    proj, dx, keep = _dev(c['proj']), _dev(c['dx']), _dev(c['keep'])
    cls_tok, mask_tok, pos, type_row, masked = _img_args(c)
    x_r, pre, sums, abs_sums = ec.img_sums(proj, cls_tok, mask_tok, pos, type_row, masked, keep, inv, dx)
    x = Guarded((B, npatch + 1, d))
    hip.embed_img_finish(proj, cls_tok, mask_tok, pos, type_row, masked, x.t, B, npatch, d, drop=c['drop'], seed=c['seed'])
    if keep is not None:
        _mask_positions('embed_img', x.t, type_row, pre, keep, inv)
    # four roundings: src + pos (its error grows by 1 / (1 - p)), 1 / (1 - p) itself to fp32, the product, + type
    _ratio('embed_img x', x.t, x_r, ec.U * (3 * (pre * inv).abs() + x_r.abs()) * (1 + 2.0 ** -20))
    x.intact('x')
    dproj = Guarded((B * npatch, d), dtype=torch.bfloat16)
    outs = {n: Guarded(s, fill=torch.zeros(s, device=DEV)) for n, s in
            {'dcls': (d,), 'dmask': (d,), 'dpos': (npatch + 1, d), 'dtype_row': (d,)}.items()}
    hip.embed_img_bwd(dx, masked, dproj.t, *[outs[n].t for n in ec.IMG_OPTIONAL], B, npatch, d, drop=c['drop'], seed=c['seed'])
    # two fp32 roundings (1 / (1 - p) itself, the product) and the bf16 one: 8 significant bits, half an ulp is 2^-8
    # relative at the most
    _ratio('dproj', dproj.t.view(B, npatch, d), sums['dproj'], abs_sums['dproj'] * (2.0 ** -8 + 3 * ec.U))
    n_masked = int(masked.sum())
    for name, key, n in (('dcls', 'img_dcls', B), ('dmask', 'img_dmask', n_masked), ('dpos', 'img_dpos', B),
                         ('dtype_row', 'img_dtype', B * (npatch + 1))):
        _ratio(name, outs[name].t, sums[name], ec.colsum_bound(key, n, abs_sums[name]))
        outs[name].intact(name)
    dproj.intact('dproj')


# ================================================================================================ d = 0
def test_d_zero_is_refused_before_any_launch():
    """vlmo_embed_img_finish, vlmo_embed_img_bwd, vlmo_embed_txt_fwd and vlmo_embed_txt_bwd refuse d = 0 with an
    argument error; the NaN-filled outputs are untouched"""
    B, n, T = 2, 3, 4
    f = lambda *s: torch.ones(*s, device=DEV)
    nan = lambda *s: torch.full(s, NAN, device=DEV)
    ids = torch.ones(B, T, dtype=torch.int64, device=DEV)
    x, xhat, rstd = nan(B * T, 4), nan(B * T, 4), nan(B * T)
    outs = [nan(8, 4), nan(T, 4), nan(4), nan(4), nan(4), nan(4)]
    dproj = torch.full((B * n, 4), NAN, device=DEV, dtype=torch.bfloat16)
    calls = {
        'vlmo_embed_img_finish': lambda: hip.embed_img_finish(f(B * n, 4).bfloat16(), f(4), f(4), f(n + 1, 4), f(4), None, x, B, n, 0),
        'vlmo_embed_img_bwd': lambda: hip.embed_img_bwd(f(B, n + 1, 4), None, dproj, *outs[2:], B, n, 0),
        'vlmo_embed_txt_fwd': lambda: hip.embed_txt_fwd(ids, f(8, 4), f(T, 4), f(4), f(4), f(4), f(4), x, xhat, rstd, B, T, 0, ec.EPS),
        'vlmo_embed_txt_bwd': lambda: hip.embed_txt_bwd(f(B * T, 4), ids, f(B * T, 4), f(B * T), f(4), *outs, B, T, 0),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match=name + ': bad shape'):
            call()
    torch.cuda.synchronize()
    for t in [x, xhat, rstd, dproj] + outs:
        assert t.isnan().all()
