"""Premises of tests/test_embedding_kernels_gpu.py, checked without a device on the case lists of tests/embed_cases.py
(the GPU file parametrises over the same lists).

Exact cases: every sum the kernels form stays far below 2^24 in sum of |terms| (so every partial sum, in any order, is
exact), every quotient and product claimed exact is exact (recomputed in fp32 and in fp64, compared bit for bit), and
the lists reach every template instance and launch regime they name.  Bounded cases: the fp32 emulation of a row, in
each of its summation orders, stays within the figures embed_cases.FIG (the GPU bound is four times those), the row
standard deviations stay above 0.1 and the mask-position check leaves out no element."""
import functools

import pytest
import torch

from tests import embed_cases as ec


def _f32_equals_f64(a32, a64):
    return a32.dtype == torch.float32 and torch.equal(a32.double(), a64)


# ------------------------------------------------------------------------------------------------ exact: text backward
@pytest.mark.parametrize('ragged', [False, True], ids=['fixed', 'ragged'])
@pytest.mark.parametrize('case', ec.TXT_EXACT, ids=ec.txt_exact_id)
def test_txt_exact_rows_are_exact_in_fp32(case, ragged):
    c = ec.txt_exact(*case, ragged=ragged)
    d, dx, xh, rs, w = c['d'], c['dx'], c['xhat'], c['rstd'], c['ln_w']
    for t in (dx, xh, rs, w):
        assert t.dtype == torch.float32
    assert xh.abs().max() <= 2 and set(w.abs().unique().tolist()) <= {1.0, 2.0} and set(rs.unique().tolist()) <= {0.5, 1.0, 2.0, 4.0}
    assert torch.equal(dx, dx.round()) and torch.equal(xh, xh.round())
    # the row in fp32, operation by operation as embed_txt_row_bwd, against fp64
    gy = dx if c['keep'] is None else torch.where(c['keep'], dx * 2.0, torch.zeros(()))
    g = gy * w
    assert (g.abs().sum(1) < 2.0 ** 24).all() and ((g * xh).abs().sum(1) < 2.0 ** 24).all()     # any partial sum of s1, s2
    s1, s2 = g.sum(1), (g * xh).sum(1)
    s1_64, s2_64 = g.double().sum(1), (g.double() * xh.double()).sum(1)
    assert _f32_equals_f64(s1, s1_64) and _f32_equals_f64(s2, s2_64)
    if d & (d - 1) == 0:
        assert (s1_64 % d == 0).all() and (s2_64 % d == 0).all()
        if c['M'] >= 8:
            assert (s1_64 != 0).any() and (s2_64 != 0).any(), 'c1 and c2 are zero everywhere: the case would not see them'
    else:
        assert (s1_64 == 0).all() and (s2_64 == 0).all()
    c1, c2 = s1 / d, s2 / d
    assert _f32_equals_f64(c1, s1_64 / d) and _f32_equals_f64(c2, s2_64 / d)
    for de32 in (rs[:, None] * (g - c1[:, None] - xh * c2[:, None]),                       # as written
                 rs[:, None] * torch.addcmul(g - c1[:, None], xh, c2[:, None], value=-1)):   # contracted
        assert _f32_equals_f64(de32, c['de'])
    assert _f32_equals_f64(gy * xh, gy.double() * xh.double())
    assert torch.equal(c['de'] * 2, (c['de'] * 2).round()), 'de is not a multiple of 1/2'
    # every sum: sum |terms| + |prefill| stays where multiples of 1/2 are exact
    for name, a in c['abs'].items():
        if name != 'word_ids' and a.numel():
            assert a.max().item() + 5 < ec.EXACT_LIMIT, name
    assert 0 not in c['sums']['word_ids'].tolist()
    assert sorted(c['lens'])[-1] == c['T'] and (c['B'] == 1 or not ragged or 1 in c['lens'])


def test_txt_exact_list_reaches_what_it_names():
    cases = ec.TXT_EXACT
    assert {ec.vpl_of(c[2]) for c in cases} == {1, 2, 3, 4}
    assert {c[2] // 4 % 64 for c in cases if ec.vpl_of(c[2]) > 1} > {0}            # a partial LAST group beyond the first
    assert {ec.rpb_of(c[0]) for c in cases} == {4, 8, 16}
    for rpb in (4, 8, 16):
        assert any(ec.rpb_of(c[0]) == rpb and c[0] % rpb and c[0] > rpb for c in cases), f'no short last chunk at rpb {rpb}'
    assert {c[0] for c in cases} == {1, 3, 5, 16, 21, 64, 70} and {c[1] for c in cases} == {1, 7, 40}
    assert {c[2] for c in cases} >= {128, 512, 1024, 768, 772}
    for d in {c[2] for c in cases}:
        assert {c[3] for c in cases if c[2] == d} == {False, True} or d in (300,), f'd = {d} runs one dropout setting only'
    hot = [int((ec.txt_exact(*c)['tok'] == c[4] - 1).sum()) for c in cases if c[0] * c[1] >= 147]
    assert max(hot) >= 64
    big = [c for c in cases if c[4] >= 30000]
    assert big and (ec.txt_exact(*big[0])['sums']['word_ids'] * big[0][2] > 2 ** 24).any()
    assert any((ec.txt_exact(*c)['tok'] == 0).any() for c in cases)


# ------------------------------------------------------------------------------------------------ exact: image
@pytest.mark.parametrize('case', ec.IMG_EXACT, ids=ec.img_exact_id)
def test_img_exact_is_exact_in_fp32(case):
    c = ec.img_exact(*case)
    B, npatch, d = c['B'], c['npatch'], c['d']
    assert torch.equal(c['proj'], c['proj'].bfloat16().float())
    mk = torch.zeros(B, npatch, 1, dtype=torch.bool) if c['masked'] is None else c['masked'].bool().unsqueeze(-1)
    src = torch.where(mk, c['mask_tok'].expand(B, npatch, d), c['proj'].view(B, npatch, d))
    v = torch.cat([c['cls_tok'].expand(B, 1, d), src], 1) + c['pos']
    if c['keep'] is not None:
        v = torch.where(c['keep'], v * 2.0, torch.zeros(()))
    assert _f32_equals_f64(v + c['type_row'], c['x'])
    g = c['sums']['dproj']
    assert torch.equal(g, g.float().bfloat16().double()), 'dproj is not exact in bf16'
    for name in ec.IMG_OPTIONAL:
        assert c['abs'][name].max().item() + 5 < ec.EXACT_LIMIT, name
        assert torch.equal(c['sums'][name], c['sums'][name].round())
    if case[3] == 'mixed':
        assert c['masked'].any() and not c['masked'].all()


def test_img_exact_list_reaches_what_it_names():
    modes = {c[3] for c in ec.IMG_EXACT}
    assert modes == {'mixed', 'none', 'zeros', 'ones'}
    for m in modes:
        assert {c[4] for c in ec.IMG_EXACT if c[3] == m} == {False, True}


# ------------------------------------------------------------------------------------------------ exact: patchify, cast
def test_patchify_shapes_and_the_grid_cap():
    over = [s for s in ec.PATCHIFY if s[0] * s[1] * s[2] * s[3] // 4 > ec.PATCHIFY_GRID_CAP * 256]
    assert over == [ec.PATCHIFY[-1]]
    B, C, H, W, p = over[0]
    assert B * C * H * W // 4 < 2 * ec.PATCHIFY_GRID_CAP * 256          # the second trip is partial
    assert {s[4] for s in ec.PATCHIFY} == {4, 16, 32} and {s[1] for s in ec.PATCHIFY} == {1, 3}
    assert any(s[2] != s[3] for s in ec.PATCHIFY) and (1, 3, 384, 384, 16) in ec.PATCHIFY
    img = torch.arange(2 * 3 * 8 * 12, dtype=torch.float32).view(2, 3, 8, 12)
    want = torch.nn.functional.unfold(img, 4, stride=4).transpose(1, 2).reshape(-1, 48)
    assert torch.equal(ec.patchify_ref(img, 4), want)


def test_cast_sources_are_exact_in_both_types_and_cover_every_alignment():
    kind = lambda n: 64 if n % 64 == 0 else (4 if n % 4 == 0 else 1)
    assert {(kind(r), kind(c)) for r, c in ec.CAST_SHAPES} == {(a, b) for a in (64, 4, 1) for b in (64, 4, 1)}
    for r, c in ec.CAST_SHAPES:
        s = ec.cast_src(r, c)
        assert torch.equal(s.bfloat16().float(), s) and torch.equal(s.half().float(), s)


# ------------------------------------------------------------------------------------------------ bounded
def _emulation_ratios(tabs, tok, pos_t, keep, inv, dx):
    """largest deviation of the emulation from fp64, per (output, order), in the units of embed_cases"""
    e, xhat, rstd, pre = ec.txt_fwd_ref(tabs, tok, pos_t)
    assert ((e - e.mean(1, keepdim=True)).square().mean(1).sqrt() >= 0.1).all(), 'a row has a standard deviation below 0.1'
    kp = 1.0 if keep is None else keep.double() * inv
    x = pre * kp + tabs[5].double()
    n_out = int(ec.left_out(pre, inv, tabs[5]).sum())
    assert n_out <= ec.LEFT_OUT_CAP * pre.numel() and n_out == 0
    ratios = {}
    xh32, rs32 = xhat.float(), rstd.float()
    for order in ec.ORDERS:
        x_e, xhat_e, rstd_e = ec.emul_row_fwd(tabs, tok, pos_t, order, keep, inv)
        ratios['x', order] = ((x_e.double() - x).abs() / ec.unit_x(x, xhat, tabs[3], tabs[4])).max().item()
        ratios['xhat', order] = ((xhat_e.double() - xhat).abs() / ec.unit_xhat(xhat)).max().item()
        ratios['rstd', order] = ((rstd_e.double() - rstd).abs() / ec.unit_rstd(rstd)).max().item()
        if dx is not None:
            _, _, de = ec.txt_bwd_sums(dx, keep, inv, xh32, rs32, tabs[3], tok, pos_t, int(pos_t.max()) + 1)
            gy = dx.double() * kp
            de_e = ec.emul_row_bwd(dx, keep, inv, xh32, rs32, tabs[3], order)
            ratios['de', order] = ((de_e.double() - de).abs() / ec.unit_de(gy * tabs[3].double(), xh32.double(), rs32.double())).max().item()
    return ratios


@functools.lru_cache(maxsize=None)
def _ratios_of(case):
    """case: an entry of BOUNDED_TXT, or the grid-cap case of a form ('cap_fixed', 'cap_rows')"""
    if isinstance(case, str):
        c, src, keep = ec.txt_cap_case(case[4:])
        return _emulation_ratios(c['tabs'], c['ids'].view(-1)[src], src % c['T'], keep, c['drop'][1], None)
    c = ec.txt_bounded(*case)
    pos_t = torch.arange(c['T']).repeat(c['B'])
    return _emulation_ratios(c['tabs'], c['ids'].view(-1), pos_t, c['keep'], c['drop'][1], c['dx'])


_BOUNDED = ec.BOUNDED_TXT + ['cap_fixed', 'cap_rows']


@pytest.mark.parametrize('case', _BOUNDED, ids=lambda c: c if isinstance(c, str) else ec.bounded_id(c))
def test_txt_bounded_emulation_stays_within_the_figures(case):
    """all three orders within FIG, so the GPU bound (MARGIN x FIG) leaves the factor 4 to spare; no element left out
    of the mask check; row standard deviations >= 0.1"""
    r = _ratios_of(case)
    print(case, {f'{k[0]}/{k[1]}': round(v, 3) for k, v in r.items()})
    for (what, order), v in r.items():
        assert v <= ec.FIG[what], f'{what}, {order} order: {v:.3f} units, embed_cases.FIG says {ec.FIG[what]}'


def test_txt_cap_case_size():
    B, T, d = ec.TXT_CAP
    assert B * T == 32772 and (B * T + 3) // 4 > ec.TXT_FWD_GRID_CAP
    for form in ('fixed', 'rows'):
        c, src, keep = ec.txt_cap_case(form)
        assert len(src) == B * T == len(keep) and int(src.max()) < c['ids'].numel() and (src[1:] > src[:-1]).all()


def test_figures_are_the_measured_ones():
    """the constants are the emulation's maxima over every case rounded up, not a guess: no more than twice them"""
    measured = {k: 0.0 for k in ec.FIG}
    for case in _BOUNDED:
        for (what, _), v in _ratios_of(case).items():
            measured[what] = max(measured[what], v)
    print('measured', measured, 'stated', ec.FIG)
    for k, v in measured.items():
        assert v <= ec.FIG[k] <= 2 * v, (k, v, ec.FIG[k])


@pytest.mark.parametrize('case', ec.BOUNDED_IMG)
def test_img_bounded_inputs(case):
    c = ec.img_bounded(*case)
    _, pre, _, _ = ec.img_sums(c['proj'], c['cls_tok'], c['mask_tok'], c['pos'], c['type_row'], c['masked'], c['keep'],
                               c['drop'][1], c['dx'])
    n_out = int(ec.left_out(pre, c['drop'][1], c['type_row']).sum())
    assert n_out == 0
    assert c['masked'].any() and not c['masked'].all()
