"""TEST INFRASTRUCTURE ONLY: case builders, fp64 references and the fp32 row emulation of the embedding kernel tests
(csrc/elementwise.hip: patchify, embed_img_finish / embed_img_bwd, embed_txt_fwd / embed_txt_bwd, the row-table pair
embed_txt_rows_* with embed_txt_fold, cast_weight).  A plain module: importing it needs neither a device nor the built
library.  tests/test_embedding_cases_cpu.py checks the premises stated here on the CPU,
tests/test_embedding_kernels_gpu.py runs the kernels on the same case lists.

Two kinds of case.

EXACT: small-integer data on which every fp32 operation of the kernels is exact, so the order of the atomics, of the
waves and FMA contraction cannot matter and the comparison with the fp64 sums is torch.equal.  Dropout runs at p = 0.5
(thresh 32 768, 1 / (1 - p) = 2).  The text backward takes xhat / rstd / ln_w as INPUTS, so they are crafted: xhat
integers in [-2, 2], rstd in {1/2, 1, 2, 4}, ln_w in {+-1, +-2}.  With g = dropout(dx) * ln_w the kernel forms c1 =
sum(g) / d, c2 = sum(g * xhat) / d and de = rstd * (g - c1 - xhat * c2).  At d a power of two the rows are corrected
(on columns with |ln_w| = 1: xhat = 0 there moves sum(g) alone, xhat = 1 moves both) until both sums are multiples of
d: c1, c2 are integers, de a multiple of 1/2.  At the other widths (300, 768, 772) the second half of a row repeats
xhat and negates g: both sums are 0 and de = rstd * g.

BOUNDED: gaussian fp32 tables.  Column sums of N terms t_i are held to (N - 1 + k) u sum|t_i| (u = 2^-24, k = fp32
roundings inside one term, K_ROUNDINGS); per-row results (x, xhat, rstd, de) to four times the largest deviation from
fp64 of an fp32 emulation of the row in three summation orders (FIG, measured by the CPU test), in the units UNIT_*.
"""
import functools
import math

import torch

from tests import dropmask

U = 2.0 ** -24
EPS = 1e-12
P_EXACT, P_BOUNDED = 0.5, 0.1
LEFT_OUT_CAP = 1e-3                 # share of a case the mask-position check may leave out
EXACT_LIMIT = 2.0 ** 22             # sum of |terms| + |prefill| of an exact sum: multiples of 1/2 below 2^23 are exact
MARGIN = 4.0                        # GPU bound = MARGIN * FIG: 1-ulp hardware rsqrt and FMA contraction are not emulated

# fp32 roundings inside ONE term of a column sum, against a reference that multiplies by the double 1 / (1 - p).
# dtype0 / dtype_row add dx as loaded.  With dropout dln_b, dcls, dmask and the image dpos add dx * fl(1 / (1 - p)): the
# factor rounded to fp32 and the product (two; none without dropout, the bound keeps two), dln_w the product of that
# with xhat (three).  The sums of de (dword rows, text dpos, dbtype0) carry the per-row bound of each term instead.
K_ROUNDINGS = {'dtype0': 0, 'dln_b': 2, 'dln_w': 3, 'img_dtype': 0, 'img_dcls': 2, 'img_dmask': 2, 'img_dpos': 2}

# Largest deviation of the fp32 row emulation (sequential, pairwise, the kernel's order) from fp64 over BOUNDED_TXT and
# TXT_CAP, in the units of unit_x / unit_xhat / unit_rstd / unit_de; tests/test_embedding_cases_cpu.py measures them and
# asserts they are not exceeded.  Taken from the emulation alone.
# Measured: x 15.03 (d = 772), xhat 13.97, rstd 16.80 (d = 1024), all three in the sequential order -- the pairwise and
# the kernel's order stay below 6.2, 3.5 and 2.2 -- and de 3.39.
FIG = {'x': 16.0, 'xhat': 14.0, 'rstd': 17.0, 'de': 3.5}


def vpl_of(d):
    """vectors of four floats per lane the text kernels are instantiated for (csrc/common.h dispatch_vpl)"""
    return min(4, (d // 4 + 63) // 64)


def rpb_of(B):
    """sequences per workgroup of vlmo_embed_txt_bwd / vlmo_embed_txt_rows_bwd"""
    return 16 if B >= 64 else (8 if B >= 16 else 4)


def _gen(*key):
    """generator seeded by a tuple of ints"""
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) & 0x7FFFFFFF)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g)


def prefill(shape, salt):
    """non-zero-mean integer pattern in [-5, 5] the accumulating outputs start from (fp32, CPU)"""
    n = int(math.prod(shape))
    return ((torch.arange(n, dtype=torch.int64) * 7 + salt) % 11 - 5).float().view(shape)


def seed_of(*key):
    """64-bit dropout seed of a case: both halves non-zero"""
    s = sum((i + 3) * 0x9E3779B97F4A7C15 * (k + 1) for i, k in enumerate(key)) & 0xFFFFFFFFFFFFFFFF
    return s | (1 << 40) | 1


# ================================================================================================ exact: text backward
# (B, T, d, dropout, V, ragged lengths or None).  B covers waves without a row (B < 4), every rows_per_block (4 below
# 16, 8 from 16, 16 from 64) and a short last chunk (5, 21, 70); d covers VPL 1 (128), 2 (300, 512), 3 (768), 4 (772,
# 1024) and a partially filled last vector group (300: 75 vectors, 772: 193).  V = 40 000 at d = 768: id * d > 2^24.
TXT_EXACT = [
    (1, 1, 128, False, 50), (1, 40, 772, False, 50), (3, 7, 128, True, 50), (3, 1, 512, True, 50),
    (5, 40, 512, False, 50), (5, 7, 300, True, 50), (16, 7, 1024, True, 50), (16, 40, 512, True, 50),
    (21, 7, 768, False, 50), (21, 40, 128, True, 50), (64, 1, 128, False, 50), (64, 7, 768, True, 40000),
    (70, 7, 1024, False, 50), (70, 40, 772, True, 50),
]


def txt_exact_id(c):
    B, T, d, drop, V = c
    short = '' if B % rpb_of(B) == 0 else '-shortchunk'
    part = '' if (d // 4) % 64 == 0 else '-partialgroup'
    return f'B{B}-T{T}-d{d}-vpl{vpl_of(d)}{part}-rpb{rpb_of(B)}{short}-{"p0.5" if drop else "nodrop"}-V{V}'


def ragged_lens(B, T, g):
    """row counts with a sample of length T and (B > 1) one of length 1"""
    lens = _ints(g, 1, T, B).tolist()
    lens[0] = T
    if B > 1:
        lens[1] = 1
    return lens


def _rows_of(B, T, lens):
    if lens is None:
        lens = [T] * B
    b = torch.tensor([bb for bb, n in enumerate(lens) for _ in range(n)], dtype=torch.int64)
    t = torch.tensor([tt for n in lens for tt in range(n)], dtype=torch.int64)
    off = torch.tensor([sum(lens[:i]) for i in range(B + 1)], dtype=torch.int32)
    return b, t, off


def _spread(total, n):
    """int64 [M] -> [M, n] integers that sum to it, as even as possible"""
    q = torch.div(total, n, rounding_mode='floor')
    r = total - q * n
    return q[:, None] + (torch.arange(n)[None, :] < r[:, None]).long()


def txt_bwd_sums(dx, keep, inv, xhat, rstd, ln_w, tok, pos_t, T):
    """fp64 restatement of embed_txt_row_bwd and the sums around it, on the device of its arguments.  dx [M, d],
    keep bool [M, d] or None, xhat / rstd / ln_w the backward's fp32 inputs, tok [M] token ids, pos_t [M] positions.
    Returns (sums, abs_sums, de): dicts with dln_w, dln_b, dtype0, dbtype0 [d], dpos [T, d], word_ids (the distinct
    non-zero ids) and dword [len(word_ids), d]; abs_sums holds sum |term| of each; de [M, d] the per-row results."""
    dx, xh, rs, w = dx.double(), xhat.double(), rstd.double()[:, None], ln_w.double()
    gy = dx if keep is None else dx * keep * inv
    g = gy * w
    d = dx.shape[1]
    c1, c2 = g.sum(1, keepdim=True) / d, (g * xh).sum(1, keepdim=True) / d
    de = rs * (g - c1 - xh * c2)
    out = []
    for f in (lambda a: a, torch.abs):
        out.append({'dln_w': f(gy * xh).sum(0), 'dln_b': f(gy).sum(0), 'dtype0': f(dx).sum(0), **fold_rows(f(de), tok, pos_t, T)})
    return out[0], out[1], de


def fold_rows(v, tok, pos_t, T):
    """sums of the rows of v [M, d] (fp64) the way de is summed: dword [len(word_ids), d] over the rows of each distinct
    non-zero id, dpos [T, d] over the rows of each position, dbtype0 [d] over all rows"""
    word_ids, inverse = torch.unique(tok, return_inverse=True)
    dword = torch.zeros(len(word_ids), v.shape[1], dtype=torch.float64, device=v.device).index_add_(0, inverse, v)
    dpos = torch.zeros(T, v.shape[1], dtype=torch.float64, device=v.device).index_add_(0, pos_t, v)
    return {'dbtype0': v.sum(0), 'dpos': dpos, 'word_ids': word_ids[word_ids != 0], 'dword': dword[word_ids != 0]}


@functools.lru_cache(maxsize=4)
def txt_exact(B, T, d, drop, V, ragged=False):
    """One exact text-backward case (CPU tensors): inputs of the kernel and the fp64 sums it must reproduce bit for
    bit.  ragged: the row-table form's packed rows (the dropout mask is indexed by the PACKED row, so the rows are
    built for it)."""
    g = _gen(B, T, d, int(drop), V, int(ragged))
    lens = ragged_lens(B, T, g) if ragged else [T] * B
    rb, rt, off = _rows_of(B, T, lens)
    M, k = len(rb), (2 if drop else 1)
    seed = seed_of(B, T, d, int(ragged))
    keep = dropmask.keep_mask(seed, M, d, dropmask.thresh_of(P_EXACT)[0]) if drop else torch.ones(M, d, dtype=torch.bool)
    rstd = 2.0 ** _ints(g, -1, 2, M).float()
    pow2 = d & (d - 1) == 0
    if pow2:
        ln_w = torch.where(torch.rand(d, generator=g) < 0.25, 2, 1) * (_ints(g, 0, 1, d) * 2 - 1)
        xh, dx = _ints(g, -2, 2, M, d), _ints(g, -8, 8, M, d)
        nc = max(4, d // 32)                        # correction columns per class
        score = torch.rand(M, d, generator=g)
        score[~(keep & (ln_w.abs() == 1)[None, :])] = -1.0
        top = score.topk(2 * nc, dim=1)
        assert (top.values > 0).all(), 'a row has too few kept columns with |ln_w| = 1'
        colA, colB = top.indices[:, :nc], top.indices[:, nc:]
        xh.scatter_(1, colA, 0)
        xh.scatter_(1, colB, 1)
        for cols, use_xh in ((colB, True), (colA, False)):          # sum(g * xhat) first, then sum(g) on xhat = 0
            gi = dx * k * keep * ln_w
            s = (gi * xh).sum(1) if use_xh else gi.sum(1)
            target = torch.div(s + d // 2, d, rounding_mode='floor') * d + _ints(g, -1, 1, M) * d
            delta = _spread(torch.div(target - s, k, rounding_mode='floor'), nc)
            assert ((target - s) % k == 0).all()
            dx.scatter_add_(1, cols, delta * ln_w[cols])            # |ln_w| = 1 there: delta * w * w = delta
    else:
        h = d // 2
        wh = torch.where(torch.rand(h, generator=g) < 0.25, 2, 1) * (_ints(g, 0, 1, h) * 2 - 1)
        ln_w = torch.cat([wh, wh])
        xhh, dxh = _ints(g, -2, 2, M, h), _ints(g, -8, 8, M, h)
        same = keep[:, :h] == keep[:, h:]                           # a pair the mask splits gets no gradient
        xh, dx = torch.cat([xhh, xhh], 1), torch.cat([dxh * same, -dxh * same], 1)
    ids = _ints(g, 1, V - 1, B, T)
    if V >= 30000:
        ids[:, 0] = _ints(g, 2 ** 24 // d + 1, V - 1, B)            # id * d > 2^24 on every first position
    tok_rows = torch.rand(M, generator=g)
    flat = ids.view(-1)
    src = rb * T + rt
    if M >= 64:
        hot = src[tok_rows.topk(max(64, M // 4)).indices]           # one id on >= 64 rows
        flat[hot] = V - 1
    if M >= 8:
        flat[src[(-tok_rows).topk(max(1, M // 10)).indices]] = 0    # padding ids inside the texts
    tok = flat[src]
    case = dict(B=B, T=T, d=d, V=V, M=M, lens=lens, maxlen=max(lens), off=off, src=src.to(torch.int32), ids=ids, tok=tok,
                pos_t=rt, seed=seed, drop=dropmask.thresh_of(P_EXACT) if drop else (0, 1.0), keep=keep if drop else None,
                dx=dx.float(), xhat=xh.float(), rstd=rstd, ln_w=ln_w.float())
    case['sums'], case['abs'], case['de'] = txt_bwd_sums(case['dx'], case['keep'], 2.0, case['xhat'], rstd, case['ln_w'],
                                                         tok, rt, T)
    return case


# ================================================================================================ exact: image
# (B, npatch, d, mask mode, dropout).  'none' is masked = None (no MIM), 'zeros' / 'ones' mask ratio 0 / 1.
IMG_EXACT = [(3, 4, 128, m, p) for m in ('mixed', 'none', 'zeros', 'ones') for p in (False, True)] + \
            [(5, 9, 300, 'mixed', True), (2, 196, 768, 'mixed', True), (2, 196, 768, 'none', False)]
IMG_OPTIONAL = ('dcls', 'dmask', 'dpos', 'dtype_row')


def img_exact_id(c):
    B, npatch, d, mode, drop = c
    return f'B{B}-np{npatch}-d{d}-masked_{mode}-{"p0.5" if drop else "nodrop"}'


def img_sums(proj, cls_tok, mask_tok, pos, type_row, masked, keep, inv, dx):
    """fp64 restatement of embed_img_finish / embed_img_bwd on the device of its arguments.  masked uint8 [B, npatch]
    or None.  Returns x [B, npatch + 1, d], the pre-dropout value, (sums, abs_sums) with dproj [B, npatch, d] (fp64,
    before the bf16 rounding), dcls, dmask, dtype_row [d], dpos [npatch + 1, d]."""
    B, n1, d = dx.shape
    mk = torch.zeros(B, n1 - 1, 1, dtype=torch.float64, device=dx.device) if masked is None else masked.double().unsqueeze(-1)
    src = proj.double().view(B, n1 - 1, d) * (1 - mk) + mask_tok.double() * mk
    pre = torch.cat([cls_tok.double().expand(B, 1, d), src], 1) + pos.double()
    kp = 1.0 if keep is None else keep.double() * inv
    x = pre * kp + type_row.double()
    g = dx.double() * kp
    out = []
    for f in (lambda a: a, torch.abs):
        out.append({'dproj': f(g[:, 1:] * (1 - mk)), 'dcls': f(g[:, 0]).sum(0), 'dmask': f(g[:, 1:] * mk).sum((0, 1)),
                    'dpos': f(g).sum(0), 'dtype_row': f(dx.double()).sum((0, 1))})
    return x, pre, out[0], out[1]


@functools.lru_cache(maxsize=4)
def img_exact(B, npatch, d, mode, drop):
    mi = ('mixed', 'none', 'zeros', 'ones').index(mode)
    g = _gen(B, npatch, d, mi, int(drop))
    seed = seed_of(B, npatch, d, mi)
    masked = {'none': None, 'zeros': torch.zeros(B, npatch, dtype=torch.uint8), 'ones': torch.ones(B, npatch, dtype=torch.uint8),
              'mixed': (torch.rand(B, npatch, generator=g) < 0.4).to(torch.uint8)}[mode]
    if mode == 'mixed':
        masked[0, 0], masked[0, 1] = 1, 0
    keep = dropmask.keep_mask(seed, B * (npatch + 1), d, dropmask.thresh_of(P_EXACT)[0]).view(B, npatch + 1, d) if drop else None
    case = dict(B=B, npatch=npatch, d=d, masked=masked, keep=keep, seed=seed,
                drop=dropmask.thresh_of(P_EXACT) if drop else (0, 1.0),
                proj=_ints(g, -8, 8, B * npatch, d).float(), cls_tok=_ints(g, -4, 4, d).float(),
                mask_tok=_ints(g, -4, 4, d).float(), pos=_ints(g, -4, 4, npatch + 1, d).float(),
                type_row=_ints(g, -4, 4, d).float(), dx=_ints(g, -8, 8, B, npatch + 1, d).float())
    case['x'], _, case['sums'], case['abs'] = img_sums(case['proj'], case['cls_tok'], case['mask_tok'], case['pos'],
                                                       case['type_row'], masked, keep, 2.0, case['dx'])
    return case


# ================================================================================================ exact: patchify, cast
# (B, C, H, W, patch).  The last one has 4 202 500 groups of four elements, above the 16 384 x 256 one trip of the grid
# covers: the grid-stride loop runs a second, partial trip.
PATCHIFY = [(2, 3, 32, 32, 4), (2, 1, 64, 64, 16), (1, 3, 32, 96, 16), (3, 3, 64, 32, 32), (1, 3, 384, 384, 16),
            (1, 1, 4100, 4100, 4)]
PATCHIFY_GRID_CAP = 16384


def patchify_ref(img, p):
    B, C, H, W = img.shape
    return img.view(B, C, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // p) * (W // p), C * p * p)


# rows x cols with each drawn from {multiple of 64, multiple of 4 only, odd}: full 16-byte pieces, the partial tile of
# 4-wide pieces, and the element path (cols % 4 != 0 for dst, rows % 4 != 0 for dstT)
CAST_SHAPES = [(64, 64), (128, 36), (100, 64), (100, 36), (33, 64), (64, 65), (33, 65), (36, 33), (1, 4), (3, 1)]
CAST_MODES = ('dst', 'dstT', 'both')


def cast_src(rows, cols):
    """fp32 [rows, cols] of multiples of 1/8 with at most 8 significant bits: exact in bf16 and in f16"""
    return _ints(_gen(rows, cols), -128, 127, rows, cols).float() / 8


# ================================================================================================ bounded: text
BOUNDED_D = (128, 300, 512, 768, 772, 1024)
BOUNDED_TXT = [(B, 16, d, drop) for d in BOUNDED_D for B in (5, 70) for drop in (False, True)]
TXT_CAP = (2731, 12, 64)            # ntok = 32 772 > 4 x 8192: the grid-stride loop of the forward runs a second trip
TXT_FWD_GRID_CAP = 8192
TXT_CAP_V = 1000
TXT_CAP_ROWS_EXTRA = 69             # the row-table form of the cap case picks its 32 772 rows from (2731 + 69) x 12 positions


def txt_cap_case(form):
    """the grid-cap case of one form ('fixed' or 'rows'), shared by the CPU premises and the GPU test: the inputs
    (txt_bounded), src int64 [32 772] = b * T + t of each packed row, and the keep mask of the packed rows"""
    B, T, d = TXT_CAP
    ntok = B * T
    c = txt_bounded(B if form == 'fixed' else B + TXT_CAP_ROWS_EXTRA, T, d, True, V=TXT_CAP_V)
    if form == 'fixed':
        src = torch.arange(ntok)
    else:
        src = torch.randperm(c['M'], generator=torch.Generator().manual_seed(1))[:ntok].sort().values
    return c, src, c['keep'][:ntok]


def bounded_id(c):
    B, T, d, drop = c
    return f'B{B}-T{T}-d{d}-vpl{vpl_of(d)}-{"p0.1" if drop else "nodrop"}'


def txt_tables(V, T, d):
    """word, pos, btype0, ln_w, ln_b, type0 (fp32, CPU).  |ln_b| >= 1/4, so the unit of x never vanishes."""
    g = _gen(V, T, d, 77)
    r = lambda *s: torch.randn(*s, generator=g)
    return [r(V, d), r(T, d), r(d), 1 + 0.1 * r(d), 0.5 + 0.25 * r(d).clamp(-1, 1), r(d)]


@functools.lru_cache(maxsize=4)
def txt_bounded(B, T, d, drop, V=None):
    """inputs of one bounded case (CPU): ids with unique tokens on the first half of the rows (their word rows hold one
    de each), repeats and padding on the rest"""
    M = B * T
    V = V or M + 50
    g = _gen(B, T, d, int(drop), 5)
    ids = (torch.randperm(V - 1, generator=g)[:M] if V > M else _ints(g, 0, V - 2, M)) + 1
    ids[M // 2:] = ids[M // 2:] % 23
    ids = ids[torch.randperm(M, generator=g)].view(B, T)
    seed = seed_of(B, T, d, 9)
    thr = dropmask.thresh_of(P_BOUNDED)
    return dict(B=B, T=T, d=d, V=V, M=M, ids=ids, tabs=txt_tables(V, T, d), seed=seed, drop=thr if drop else (0, 1.0),
                keep=dropmask.keep_mask(seed, M, d, thr[0]) if drop else None, dx=torch.randn(M, d, generator=g))


def txt_fwd_ref(tabs, tok, pos_t):
    """fp64 LayerNorm(word + btype0 + pos) of rows (tok, pos_t): e, xhat, rstd, pre = ln_w xhat + ln_b"""
    word, pos, bt0, lw, lb, _ = [t.double() for t in tabs]
    e = word[tok] + bt0 + pos[pos_t]
    mu = e.mean(1, keepdim=True)
    rstd = ((e - mu).square().mean(1) + EPS).rsqrt()
    xhat = (e - mu) * rstd[:, None]
    return e, xhat, rstd, xhat * lw + lb


def unit_x(x, xhat, ln_w, ln_b):
    return U * (x.abs() + (ln_w.double() * xhat).abs() + ln_b.double().abs())


def unit_xhat(xhat):
    return U * (xhat.abs() + 1)


def unit_rstd(rstd):
    return U * rstd.abs()


def unit_de(g, xhat, rstd):
    """g = dropout(dx) * ln_w (fp64), xhat / rstd the backward's inputs.  The two row means enter with the sum of the
    magnitudes they add up, not with their (cancelled) value: that is the scale of a summation error."""
    d = g.shape[1]
    a1, a2 = g.abs().sum(1, keepdim=True) / d, (g * xhat).abs().sum(1, keepdim=True) / d
    return U * rstd[:, None] * (g.abs() + a1 + xhat.abs() * a2)


# ---- fp32 emulation of a row in three summation orders
def _sum_seq(x):
    s = x[:, 0].clone()
    for c in range(1, x.shape[1]):
        s += x[:, c]
    return s


def _sum_pair(x):
    n = 1 << (x.shape[1] - 1).bit_length()
    x = torch.cat([x, x.new_zeros(x.shape[0], n - x.shape[1])], 1)
    while x.shape[1] > 1:
        x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def _wave_sum(s):
    """csrc/common.h wave_sum on [rows, 64]: quads by row_shr 1..3, then 4, 8 inside a row of 16, then the row
    broadcasts; the value lane 63 ends with"""
    s = s.view(-1, 4, 4, 4)                                          # [rows, dpp row, quad, lane of the quad]
    q = ((s[..., 3] + s[..., 2]) + s[..., 1]) + s[..., 0]            # lane 4q + 3: v + shr1 + shr2 + shr3
    r = (q[..., 3] + q[..., 2]) + (q[..., 1] + q[..., 0])            # lane 15 of a row
    return (r[:, 3] + r[:, 2]) + (r[:, 1] + r[:, 0])


def _sum_kernel(x, grouped):
    """the text kernels' order: lane l of 64 holds vector i = l + 64 j (four columns), j ascending; `grouped` adds a
    vector as ((a + b) + c) + d to the lane's sum (the mean), otherwise column by column (the other sums)"""
    rows, d = x.shape
    vpl = (d // 4 + 63) // 64
    x = torch.cat([x, x.new_zeros(rows, vpl * 256 - d)], 1).view(rows, vpl, 64, 4)
    s = x.new_zeros(rows, 64)
    for j in range(vpl):
        if grouped:
            s = s + (((x[:, j, :, 0] + x[:, j, :, 1]) + x[:, j, :, 2]) + x[:, j, :, 3])
        else:
            for k in range(4):
                s = s + x[:, j, :, k]
    return _wave_sum(s)


ORDERS = ('sequential', 'pairwise', 'kernel')


def _sum(x, order, grouped=False):
    return {'sequential': _sum_seq, 'pairwise': _sum_pair}[order](x) if order != 'kernel' else _sum_kernel(x, grouped)


def emul_row_fwd(tabs, tok, pos_t, order, keep=None, inv=1.0):
    """fp32 emulation of embed_txt_row: mean, centred variance, rsqrt, the affine step, dropout, + type0"""
    word, pos, bt0, lw, lb, t0 = tabs
    d = word.shape[1]
    e = (word[tok] + bt0) + pos[pos_t]
    mu = (_sum(e, order, True) / d)[:, None]
    c = e - mu
    rstd = ((_sum(c * c, order) / d + torch.tensor(EPS, dtype=torch.float32)).double().rsqrt()).float()   # correctly rounded rsqrt
    xhat = c * rstd[:, None]
    o = xhat * lw + lb
    if keep is not None:
        o = torch.where(keep, o * torch.tensor(inv, dtype=torch.float32), torch.zeros(()))
    return o + t0, xhat, rstd


def emul_row_bwd(dx, keep, inv, xhat, rstd, ln_w, order):
    """fp32 emulation of embed_txt_row_bwd's de"""
    d = dx.shape[1]
    gy = dx if keep is None else torch.where(keep, dx * torch.tensor(inv, dtype=torch.float32), torch.zeros(()))
    g = gy * ln_w
    c1, c2 = (_sum(g, order) / d)[:, None], (_sum(g * xhat, order) / d)[:, None]
    return rstd[:, None] * ((g - c1) - xhat * c2)


def left_out(pre, inv, type0):
    """elements of a forward whose kept value vanishes beside the type row in fp32 (x == type0 although kept)"""
    return (pre * inv).abs() < 2.0 ** -22 * type0.double().abs()


def colsum_bound(name, n_terms, abs_sum):
    """(N - 1 + k) u sum|t_i|"""
    return (n_terms - 1 + K_ROUNDINGS[name]) * U * abs_sum


# ================================================================================================ bounded: image
BOUNDED_IMG = [(5, 9, 300, True), (3, 196, 768, False), (70, 4, 128, True)]


@functools.lru_cache(maxsize=4)
def img_bounded(B, npatch, d, drop):
    g = _gen(B, npatch, d, int(drop), 11)
    r = lambda *s: torch.randn(*s, generator=g)
    seed = seed_of(B, npatch, d, 13)
    thr = dropmask.thresh_of(P_BOUNDED)
    masked = (torch.rand(B, npatch, generator=g) < 0.4).to(torch.uint8)
    masked[0, 0], masked[0, 1] = 1, 0
    return dict(B=B, npatch=npatch, d=d, masked=masked, seed=seed, drop=thr if drop else (0, 1.0),
                keep=dropmask.keep_mask(seed, B * (npatch + 1), d, thr[0]).view(B, npatch + 1, d) if drop else None,
                proj=r(B * npatch, d).bfloat16(), cls_tok=r(d), mask_tok=r(d), pos=r(npatch + 1, d), type_row=r(d),
                dx=r(B, npatch + 1, d))
