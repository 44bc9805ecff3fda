"""Peaked-score inputs for the training path's attention kernels (csrc/attention.hip), their fp64 reference, derived
per-element error bounds and the premises each case exists for.  A plain module: importing it
needs no device, every function takes the device to work on.

Inputs.  qkv = Gaussian + a rank-one term: with e = 1 on the first 16 features of a head, q_i = x_i + a_i e and
k_j = y_j + r_j e, so the scaled score (scale = 1 / 8) is 2 a_i r_j + noise of about unit size.  All arithmetic below is
on the bf16-rounded values.

Bounds (fp64, u = 2^-8 the unit roundoff of bf16; P~ = P * keep * inv_keep).  The kernels round P, dS and every output
to bf16 once each and take delta from the bf16 ctx:
    ctx    2u sum_j P~_ij |v_jd|
    delta  D_i  = 2u sum_d |dO_id| sum_j P~_ij |v_jd|
    dS     E_ij = 2u |dS_ij| + P_ij D_i
    dq     scale sum_j E_ij |k_jd|        dk   scale sum_i E_ij |q_id|        dv   2u sum_i P~_ij |dO_id|
    qv     the sum of the row bounds of the sequence
Each takes an additive fp32 term: 2u becomes 2u + 2 eta_f where the forward's probabilities enter (ctx, D) and
2u + eta_b where the backward's do (dv, the first term of E), eta the relative fp32 error of a probability (fp32_eta),
plus TINY for fp32 underflow."""
import math

import torch

from tests import attn_counter

SCALE = 64 ** -0.5
U = 2.0 ** -8                   # unit roundoff of bf16
TINY = 1e-30                    # probabilities below the smallest normal fp32 (1.2e-38) flush to zero: <= 1024 terms of
                                # them times operands below 2^10 stay under this
LAZY_THR = 8.0 * math.log(2.0)  # the lazy-rescale threshold of attn_fwd1_kernel (8 in log2 units) in scaled score units
# lse tolerance a + b |lse|: four times the worst error of the fp32 emulation of the kernels' own lse formulas
# (tests/attn_emul.py) against fp64 over every case below, measured on the CPU before any GPU run:
# 1.05e-6 on the rows with |lse| <= 8 and 7.24e-7 |lse| on the others (the 64 roundings of a score of 2^9 .. 2^10 raw units
# are most of it), both forms alike.  The factor 4 stands for v_exp_f32 / v_log_f32 at 1 ulp each against libm.
LSE_A = 4 * 1.1e-6
LSE_B = 4 * 7.3e-7

LENGTHS = (64, 256, 257, 261, 288, 289, 512, 513, 577)
MIXED_LAUNCHES = ((261, 64, 200), (577, 300, 40))


def npad(n):
    return ((n + 31) // 32) * 32


def lse_tol(lse):
    return LSE_A + LSE_B * lse.abs()


# ---------------------------------------------------------------------------------------------------------- inputs
def _r_saw(n, g):
    """key offsets: the row maximum of an a = +2 query grows by about g scaled units per 32-key tile; a sawtooth of
    period 9 tiles keeps raw scores below about 2^9 for longer sequences"""
    return g * ((torch.arange(n) // 32) % 9).float() / 4


def _pattern(pattern, n, g, spike_at):
    """(a [n], r [n]) of one sequence"""
    i = torch.arange(n)
    two = torch.full((n,), 2.0)
    if pattern == 'flat':
        return torch.zeros(n), torch.zeros(n)
    if pattern == 'rise':
        return two, _r_saw(n, g)
    if pattern == 'fall':
        return -two, _r_saw(n, g)
    if pattern == 'mixed':
        return torch.tensor([2.0, -2.0, 0.0])[(i % 3 + i % 5) % 3], _r_saw(n, g)
    if pattern == 'spike':
        r = torch.zeros(n)
        r[spike_at] = 16.0
        return two, r
    if pattern == 'low':
        return two, torch.full((n,), -12.5)
    raise ValueError(pattern)


class Case:
    """One launch: packed bf16 qkv [M, 3d] and dctx [M, d], seg [nseq][4], keymask [M], all on `device`.  Rows that no
    sequence uses hold NaN.  spike: per sequence the token of the spike key (or None)."""

    def __init__(self, name, pattern, lens, heads, mask, drop, seed, device, g=7.0, exact=None):
        self.name, self.pattern, self.lens, self.heads, self.mask, self.drop = name, pattern, list(lens), heads, mask, drop
        self.device, self.d, self.max_len = device, heads * 64, max(lens)
        d = self.d
        # a 261-token sequence is packed from a 64-row text range and a 197-row image range; all first ranges lie in
        # front, five unused rows separate them from the second ranges
        first = [64 if n == 261 else n for n in self.lens]
        seg, row = [], 0
        for n1 in first:
            seg.append([row, n1, 0, 0])
            row += n1
        row += 5
        for s, (n, n1) in enumerate(zip(self.lens, first)):
            if n > n1:
                seg[s][2], seg[s][3] = row, n - n1
                row += n - n1
        self.M = M = row
        gen = torch.Generator().manual_seed(seed)
        qkv = torch.full((M, 3 * d), float('nan'))
        dctx = torch.full((M, d), float('nan'))
        keymask = torch.ones(M, dtype=torch.int32)
        self.spike, self.rows = [], []
        for s, n in enumerate(self.lens):
            rows = torch.cat([torch.arange(seg[s][0], seg[s][0] + seg[s][1]), torch.arange(seg[s][2], seg[s][2] + seg[s][3])])
            self.rows.append(rows)
            x = torch.randn(n, 3 * d, generator=gen)
            do = torch.randn(n, d, generator=gen)
            km = torch.ones(n, dtype=torch.int32)
            spike_at = None
            if pattern == 'spike':      # token 0, token n - 1 (the fringe tile at 257 .. 288), a masked token of the last tile
                spike_at = (0, n - 1, max(n - 3, 1))[s % 3]
                if s % 3 == 2:
                    km[spike_at] = 0
            self.spike.append(spike_at)
            if exact is None:
                a, r = _pattern(pattern, n, g, spike_at)
                for hd in range(heads):
                    x[:, hd * 64:hd * 64 + 16] += a[:, None]
                    x[:, d + hd * 64:d + hd * 64 + 16] += r[:, None]
            else:
                x, do, km = exact(s, n, d, gen)
            if mask == 'tail' and n >= 64:          # the padded tail of a text range
                km[40 + 3 * s:64] = 0
            elif mask == 'tile' and n >= 128:       # one whole key tile, and the tail
                km[64:96] = 0
                km[n - 7:n - 2] = 0
            elif mask == 'first':                   # the whole first tile: the first live maximum arrives in tile 1
                km[0:32] = 0
            qkv[rows], dctx[rows], keymask[rows] = x, do, km
        self.qkv = qkv.to(torch.bfloat16).to(device)
        self.dctx = dctx.to(torch.bfloat16).to(device)
        self.keymask = keymask.to(device)
        self.seg = torch.tensor(seg, dtype=torch.int32).to(device)
        self.rows = [r.to(device) for r in self.rows]
        self.used = torch.cat(self.rows)

    def keep(self, seed, thresh):
        return attn_counter.keep_mask(seed, self.lens, self.heads, thresh)


DROP_SEED = 0x5EEDFACE0123


def case_table():
    """[(name, kwargs of Case)]: the cases of DESIGN.md 4p, shared by the CPU and the GPU tests"""
    out = []

    def add(pattern, lens, heads, mask='tail', drop=False):
        name = f"{pattern}-{'_'.join(map(str, lens))}-h{heads}-{mask}{'-drop' if drop else ''}"
        out.append((name, dict(pattern=pattern, lens=lens, heads=heads, mask=mask, drop=drop, seed=1000 + len(out))))

    for n in LENGTHS:
        heads = 2 if n <= 288 else 1
        add('rise', (n,), heads)
        add('fall', (n,), heads)
        add('mixed', (n,), heads, mask='tile')
    for lens in MIXED_LAUNCHES:
        for pattern in ('rise', 'fall', 'mixed'):
            add(pattern, lens, 1, mask='tile' if pattern == 'mixed' else 'tail')
    for n in (64, 261, 289, 513):
        add('spike', (n, n, n), 1, mask='none')
        add('low', (n,), 2)
        add('rise', (n,), 2 if n <= 288 else 1, drop=True)
        add('mixed', (n,), 2 if n <= 288 else 1, mask='tile', drop=True)
    for n in (261, 513):
        add('rise', (n,), 1, mask='first')
    return out


def make_case(name, device, **kw):
    return Case(name, device=device, **kw)


# ------------------------------------------------------------------------------------------------------- reference
def fp32_eta(ref_heads, scale=SCALE):
    """(eta_f, eta_b): bounds of the relative error of a probability as the kernels form it in fp32 against the exact
    one, in the forward (p = exp2(c q.k - m), normalised by its own row sum) and in the backward
    (p = exp2(c (q.k - lse / scale)), lse read back).  DESIGN.md 4p:
      * the score is an fp32 sum of 64 exact bf16 products onto an initial accumulator t0 (0 in the forwards and the
        streaming backward, -lse / scale in the single-pass backward): 64 roundings of partial sums, each at most
        2^-24 of its partial sum, and every partial sum lies in [t0 - neg, t0 + pos] (pos / neg: the sums of the
        positive / negative products), so with A = max_ij max(|t0 - neg|, |t0 + pos|) the error is <= 64 * 2^-24 * A in
        raw units, times scale in the exponent;
      * the argument of exp2 (one multiply, one add, each 2^-24 of at most A scale log2e) adds 2 * 2^-24 * A scale, and
        exp2 itself (v_exp_f32, 1 ulp) 2^-23; the forward's row sum of 1024 terms at most and its division 2^-22 more;
      * the lse round trip, backward only: the stored value is off by at most lse_tol.
    A probability of the forward after normalisation is off by 2 eta_f (its own error and the row sum's)."""
    Af, Ab, L = 0.0, 0.0, 0.0
    for h in ref_heads:
        q, k = h['q'], h['k']
        qp, qn, kp, kn = q.clamp(min=0), (-q).clamp(min=0), k.clamp(min=0), (-k).clamp(min=0)
        pos = qp @ kp.T + qn @ kn.T
        neg = qp @ kn.T + qn @ kp.T
        t0 = (-h['lse'] / scale)[:, None]
        Af = max(Af, torch.maximum(pos, neg).max().item())
        Ab = max(Ab, torch.maximum((t0 - neg).abs(), (t0 + pos).abs()).max().item(), Af)
        L = max(L, h['lse'].abs().max().item())
    eta_f = scale * Af * 2.0 ** -24 * 66 + 2.0 ** -23 + 2.0 ** -22
    eta_b = scale * Ab * 2.0 ** -24 * 66 + 2.0 ** -23 + LSE_A + LSE_B * L
    return eta_f, eta_b


def reference(case, keep=None, inv_keep=1.0, scale=SCALE):
    """fp64 torch per sequence and head on the case's device.  Returns a dict: ctx, dq, dk, dv [M, d] and their bounds
    b_ctx .. b_dv, lse [nseq * heads, npad(max_len)] (NaN past a sequence's length), qv / b_qv [nseq, 2d] (column sums of
    dq | dv), eta, and heads: per (sequence, head) the scaled scores S (-inf on masked keys), P, q, k, lse."""
    dev, d, H = case.device, case.d, case.heads
    M = case.M
    X = case.qkv.double()
    dO_all = case.dctx.double()
    out = {n: torch.zeros(M, d, dtype=torch.float64, device=dev) for n in
           ('ctx', 'dq', 'dk', 'dv', 'b_ctx', 'b_dq', 'b_dk', 'b_dv')}
    lse = torch.full((len(case.lens) * H, npad(case.max_len)), float('nan'), dtype=torch.float64, device=dev)
    heads = []
    for s, rows in enumerate(case.rows):
        n = len(rows)
        live = case.keymask[rows].bool()
        for hd in range(H):
            c = slice(hd * 64, hd * 64 + 64)
            q, k, v, dO = X[rows][:, c], X[rows][:, d:2 * d][:, c], X[rows][:, 2 * d:][:, c], dO_all[rows][:, c]
            S = (q @ k.T) * scale
            S = S.masked_fill(~live[None, :], float('-inf'))
            l = torch.logsumexp(S, dim=1)
            P = torch.exp(S - l[:, None])
            kf = keep[s, hd, :n, :n].to(dev).double() * inv_keep if keep is not None else torch.ones_like(P)
            Pt = P * kf
            ctx = Pt @ v
            pav = Pt @ v.abs()
            dP = dO @ v.T
            delta = (dO * ctx).sum(1)
            dS = P * (kf * dP - delta[:, None])
            heads.append(dict(S=S, P=P, q=q, k=k, lse=l, seq=s, head=hd, pav=pav, dO=dO, dS=dS, Pt=Pt, v=v, rows=rows))
            col = torch.arange(hd * 64, hd * 64 + 64, device=dev)
            ix = (rows[:, None], col[None, :])
            out['ctx'][ix], out['dq'][ix], out['dk'][ix], out['dv'][ix] = ctx, scale * (dS @ k), scale * (dS.T @ q), Pt.T @ dO
            lse[s * H + hd, :n] = l
    # the bounds, once the fp32 terms of the case are known: 2u -> 2u + 2 eta_f where the forward's probabilities enter
    # (ctx, and delta through it), 2u -> 2u + eta_b where the backward's do (P in dv, dS)
    eta_f, eta_b = fp32_eta(heads, scale)
    uf, ub = 2 * U + 2 * eta_f, 2 * U + eta_b
    for h in heads:
        col = torch.arange(h['head'] * 64, h['head'] * 64 + 64, device=dev)
        ix = (h['rows'][:, None], col[None, :])
        D = uf * (h['dO'].abs() * h['pav']).sum(1)
        E = ub * h['dS'].abs() + h['P'] * D[:, None]
        out['b_ctx'][ix] = uf * h['pav'] + TINY
        out['b_dq'][ix] = scale * (E @ h['k'].abs()) + TINY
        out['b_dk'][ix] = scale * (E.T @ h['q'].abs()) + TINY
        out['b_dv'][ix] = ub * (h['Pt'].T @ h['dO'].abs()) + TINY
        for key in ('pav', 'dO', 'dS', 'Pt', 'v', 'rows'):
            del h[key]
    out['qv'] = torch.stack([torch.cat([out['dq'][r].sum(0), out['dv'][r].sum(0)]) for r in case.rows])
    out['b_qv'] = torch.stack([torch.cat([out['b_dq'][r].sum(0), out['b_dv'][r].sum(0)]) for r in case.rows])
    out.update(lse=lse, heads=heads, eta_f=eta_f, eta_b=eta_b)
    return out


# -------------------------------------------------------------------------------------------------------- checking
def ratios(got, ref, case):
    """worst |error| / bound per output over the rows the case uses, and the worst lse error over its tolerance.
    got: dict with ctx [M, d], lse [nseq * heads, >= npad], dqkv [M, 3d], qv [nseq, 2d]."""
    d, u = case.d, case.used
    g = {k: v.double() for k, v in got.items()}
    out = {}
    pairs = (('ctx', g['ctx'], 'ctx'), ('dq', g['dqkv'][:, :d], 'dq'), ('dk', g['dqkv'][:, d:2 * d], 'dk'),
             ('dv', g['dqkv'][:, 2 * d:], 'dv'))
    for name, x, key in pairs:
        r = (x[u] - ref[key][u]).abs() / ref['b_' + key][u]
        out[name] = float('inf') if r.isnan().any() else r.max().item()
    r = (g['qv'] - ref['qv']).abs() / ref['b_qv']
    out['qv'] = float('inf') if r.isnan().any() else r.max().item()
    want = ref['lse']
    have = g['lse'][:, :want.shape[1]]
    ok = ~want.isnan()
    r = (have[ok] - want[ok]).abs() / lse_tol(want[ok])
    out['lse'] = float('inf') if r.isnan().any() else r.max().item()
    return out


def floors(got, ref, case):
    """the suite's earlier bounds (tests/test_kernels_gpu.py) as worst |error| / bound: ctx 1e-2 + |ref| / 64, dqkv
    2e-2 max|ref| + |ref| / 32 with one maximum over the three thirds, qv with the sqrt(rows) factor"""
    d, u = case.d, case.used
    out = {}
    ctx = got['ctx'].double()
    out['ctx'] = ((ctx[u] - ref['ctx'][u]).abs() / (1e-2 + ref['ctx'][u].abs() / 64)).max().item()
    rd = torch.cat([ref['dq'], ref['dk'], ref['dv']], 1)[u]
    m = rd.abs().max().item()
    r = (got['dqkv'].double()[u] - rd).abs() / (2e-2 * m + rd.abs() / 32)
    out['dqkv'] = float('inf') if r.isnan().any() else r.max().item()
    worst = 0.0
    for s, rows in enumerate(case.rows):
        r = (got['qv'][s].double() - ref['qv'][s]).abs() / (2e-2 * m * max(1.0, len(rows) ** 0.5) + ref['qv'][s].abs() / 32)
        worst = max(worst, float('inf') if r.isnan().any() else r.max().item())
    out['qv'] = worst
    return out


def assert_within(got, ref, case, what=''):
    """every per-element bound, the lse tolerance and the earlier floors; returns the ratios for the record"""
    r, f = ratios(got, ref, case), floors(got, ref, case)
    print(f'{what or case.name}: error / bound ' + ' '.join(f'{k} {v:.3f}' for k, v in r.items()) +
          ' | error / floor ' + ' '.join(f'{k} {v:.3f}' for k, v in f.items()) + f' | fp32 / bf16 term fwd {ref["eta_f"] / U:.3f} bwd {ref["eta_b"] / (2 * U):.3f}')
    bad = [f'{k} {v:.3f}' for k, v in r.items() if not v <= 1.0] + [f'floor {k} {v:.3f}' for k, v in f.items() if not v <= 1.0]
    assert not bad, f'{what or case.name}: worst error over its bound above 1: ' + ', '.join(bad)
    return r


# -------------------------------------------------------------------------------------------------------- premises
def lazy_rescales(S, n):
    """Replay of the lazy-maximum rule of attn_fwd1_kernel on scaled fp64 scores S [n, n] (-inf on masked keys), per
    32-query wave and 32-key tile: the wave rescales when some row's tile maximum exceeds its reference maximum by
    more than LAZY_THR, and then every row takes max(reference, tile maximum).  Returns (count, split): count[w] the
    rescales of wave w after its first (the first meets no accumulated value), split whether some such rescale had a
    row with alpha == 1 beside a row with alpha < 2^-8."""
    nt = (n + 31) // 32
    counts, split = [], False
    for w in range(nt):
        rows = S[w * 32:min(w * 32 + 32, n)]
        m = torch.full((rows.shape[0],), float('-inf'), dtype=S.dtype, device=S.device)
        cnt = 0
        for t in range(nt):
            mx = rows[:, t * 32:min(t * 32 + 32, n)].max(1).values
            if bool(((mx - m) > LAZY_THR).any()):
                m_new = torch.maximum(m, mx)
                started = ~m.isinf()
                if bool(started.any()):
                    cnt += 1
                    alpha = torch.exp(m - m_new)[started]
                    split = split or (bool((alpha == 1).any()) and bool((alpha < 2.0 ** -8).any()))
                m = m_new
        counts.append(cnt)
    return counts, split


def assert_premises(case, ref):
    """the property each family exists for, on the fp64 scores; returns a short record"""
    assert ref['eta_f'] <= U / 10 and ref['eta_b'] <= 2 * U / 10, \
        f'{case.name}: fp32 terms {ref["eta_f"]:.3g} / {ref["eta_b"]:.3g} above a tenth of the bf16 terms: the score range is too wide'
    rec = {}
    pmax = torch.cat([h['P'].max(1).values for h in ref['heads']])
    rec['median_pmax'] = pmax.median().item()
    per_head = [lazy_rescales(h['S'], h['S'].shape[0]) for h in ref['heads']]
    rec['rescales'] = max(max(c) for c, _ in per_head)
    p = case.pattern
    if p in ('rise', 'fall', 'mixed', 'spike'):
        assert rec['median_pmax'] >= 0.1, f'{case.name}: median largest probability {rec["median_pmax"]:.3f}'
    if p == 'rise':
        for h, (c, _) in zip(ref['heads'], per_head):
            nt = min((h['S'].shape[0] + 31) // 32, 9)          # the first period of the sawtooth
            live_tiles = sum(bool((~h['S'][0, t * 32:t * 32 + 32].isinf()).any()) for t in range(nt))
            assert max(c) >= live_tiles - 1, (case.name, c)
    if p == 'fall':
        assert rec['rescales'] == 0, (case.name, [c for c, _ in per_head])
    if p == 'mixed':
        assert all(sp for (_, sp), h in zip(per_head, ref['heads']) if h['S'].shape[0] > 32), case.name
    if p == 'spike':
        for h in ref['heads']:
            S, j = h['S'], case.spike[h['seq']]
            if S[0, j].isinf():         # the masked spike: it would have been the maximum of every row
                qk = (h['q'] @ h['k'][j]) * SCALE
                assert bool((qk > S.max(1).values + 20).all()), case.name
            else:
                rest = S.clone()
                rest[:, j] = float('-inf')
                assert (S[:, j] - rest.max(1).values).min().item() >= 30, case.name
    if p == 'low':
        top = max(h['S'].max().item() for h in ref['heads'])
        mid = torch.cat([h['S'][~h['S'].isinf()] for h in ref['heads']]).median().item()
        assert top < -20 and -55 < mid < -45, (case.name, top, mid)
        rec['top_score'] = top
    return rec


# ----------------------------------------------------------------------------------------------------- exact cases
def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def one_live_key_case(n, device, heads=1, seed=7):
    """three sequences of n tokens, one live key each: in tile 0, in the last full tile, in the last (fringe) tile.
    v holds small integers and dO is in {-1, 0, 1}: every sum of the test is exact."""
    last_full = (n // 32) * 32 - 7
    live = [5, last_full, n - 1 if n % 32 else n - 3]

    def exact(s, n_, d, gen):
        x = torch.randn(n_, 3 * d, generator=gen)
        x[:, 2 * d:] = _ints((n_, d), -3, 3, gen)
        do = _ints((n_, d), -1, 1, gen)
        km = torch.zeros(n_, dtype=torch.int32)
        km[live[s]] = 1
        return x, do, km

    c = Case(f'one-live-key-{n}', 'exact', (n, n, n), heads, 'none', False, seed, device, exact=exact)
    c.live = live
    return c


def uniform_case(device, n=261, heads=1, seed=9):
    """q = 0 and 64 live keys among n (62 in the full tiles, two in the fringe): every probability is 2^-6.  v and dO
    hold small integers."""
    live = [j for j in range(248) if j % 4 == 1] + [257, 260]
    assert len(live) == 64

    def exact(s, n_, d, gen):
        x = torch.randn(n_, 3 * d, generator=gen)
        x[:, :d] = 0
        x[:, 2 * d:] = _ints((n_, d), -3, 3, gen)
        do = _ints((n_, d), -1, 1, gen)
        km = torch.zeros(n_, dtype=torch.int32)
        km[live] = 1
        return x, do, km

    c = Case(f'uniform-{n}', 'exact', (n,), heads, 'none', False, seed, device, exact=exact)
    c.live = live
    return c


def _thirds(got, case):
    d = case.d
    x = got['dqkv'].double()
    return x[:, :d], x[:, d:2 * d], x[:, 2 * d:]


def check_one_live_key(got, ref, case):
    """no tolerance on the exact outputs: ctx rows bitwise the live key's v row, dv of the live key the integer column
    sum of dO, dv / dk of every other key and (v and dO being integers, dP == delta) all of dq / dk zero; lse the scaled
    score within its tolerance; everything within the bounds besides"""
    d = case.d
    dq, dk, dv = _thirds(got, case)
    for s, rows in enumerate(case.rows):
        j = rows[case.live[s]]
        v_row = case.qkv[j, 2 * d:]
        assert torch.equal(got['ctx'][rows].to(torch.bfloat16).view(torch.int16),
                           v_row.expand(len(rows), d).contiguous().view(torch.int16)), f'{case.name}: ctx of sequence {s}'
        colsum = case.dctx[rows].double().sum(0)
        assert colsum.abs().max().item() <= 256, 'the column sums of dO are not representable in bf16'
        assert torch.equal(dv[j], colsum), f'{case.name}: dv of the live key of sequence {s}'
        others = rows[torch.arange(len(rows), device=rows.device) != case.live[s]]
        assert bool((dv[others] == 0).all()) and bool((dk[rows] == 0).all()) and bool((dq[rows] == 0).all()), \
            f'{case.name}: a gradient that is exactly zero is not, sequence {s}'
        assert torch.equal(got['qv'][s].double(), torch.cat([torch.zeros_like(colsum), colsum])), f'{case.name}: qv of sequence {s}'
        for hd in range(case.heads):
            c = slice(hd * 64, hd * 64 + 64)
            score = (case.qkv[rows][:, c].double() @ case.qkv[j, d:2 * d][c].double()) * SCALE
            have = got['lse'][s * case.heads + hd, :len(rows)].double()
            assert bool(((have - score).abs() <= lse_tol(score)).all()), f'{case.name}: lse of sequence {s}'
    return assert_within(got, ref, case)


def check_uniform(got, ref, case):
    """ctx the exact mean of the 64 live v rows (representable: an integer of at most 8 bits over 64), lse = ln 64 within
    its tolerance, dk zero, dv of the live keys 2^-6 times the integer column sum of dO; dq within its bound"""
    d = case.d
    dq, dk, dv = _thirds(got, case)
    rows = case.rows[0]
    live = rows[torch.tensor(case.live, device=rows.device)]
    vsum = case.qkv[live, 2 * d:].double().sum(0)
    colsum = case.dctx[rows].double().sum(0)
    assert vsum.abs().max().item() <= 256 and colsum.abs().max().item() <= 256, 'the sums are not representable in bf16'
    assert torch.equal(got['ctx'][rows].double(), (vsum / 64).expand(len(rows), d)), f'{case.name}: ctx'
    assert bool((dk[rows] == 0).all()), f'{case.name}: dk'
    assert torch.equal(dv[live], (colsum / 64).expand(64, d)), f'{case.name}: dv of the live keys'
    dead = torch.ones(len(rows), dtype=torch.bool, device=rows.device)
    dead[case.live] = False
    assert bool((dv[rows[dead]] == 0).all()), f'{case.name}: dv of the masked keys'
    have = got['lse'][:case.heads, :len(rows)].double()
    want = torch.full_like(have, math.log(64.0))
    assert bool(((have - want).abs() <= lse_tol(want)).all()), f'{case.name}: lse'
    return assert_within(got, ref, case)
