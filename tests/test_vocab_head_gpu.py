"""The vocabulary head, element by element: the chunked epilogues VLMO_EPI_CE / VLMO_EPI_ARGMAX (csrc/gemm_common.h),
their folds vlmo_ce_reduce / vlmo_argmax_reduce (csrc/dvae.hip), the recomputing backward VLMO_EPI_CE_BWD and
heads.LinearCrossEntropyFn end to end, each against fp64 on the CPU.

Kernel-level cases use exact-integer operands (A, B in {-1, 0, 1}, K = 64, bias (column % 7) - 3): every logit is an
integer, exact in fp32, bf16 and f16, so chunk maxima, arg-maxima and label logits must equal the reference bit for
bit, and tied maxima (the lowest index wins) occur without being constructed -- each test asserts that they do.  The
sizes are those at which the chunk bookkeeping changes: an odd number of 64-column chunks (a wave of the 128- or
256-wide tile lies wholly past N), 65 chunks (the folds' lane loop wraps), vocabularies that are no multiple of 64, 1,
5 and 130 rows (fewer rows than a fold block, waves wholly past M), and the production width 30 528.

Every partial buffer is written twice: once with a spare column (ldo = chunks + 1) and once in the production layout
(ldo = chunks), each with spare rows behind it, all prefilled with a NaN pattern.  Nothing outside the real elements may
change, no real element may keep the pattern, and the two layouts and a repeat must agree bit for bit."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'

from exploremultimodal_amd import hip  # noqa: E402

K = 64
POOL = 146                  # rows of a case's pool; the M-row cases take its first M rows
PAD = 6                     # the CE cases leave the last 6 columns to the padding of the bf16 head copies (30 522 -> 30 528)
SPARE = 4                   # guard rows behind a partial buffer (>= one 256-wide tile of chunks even at ldo = 1)
SENTINEL = 0x7FC0DEAD       # a quiet-NaN bit pattern no kernel result can equal (not a column index, not a sum)
CE_SHAPES = [(N, M) for N in (64, 192, 320, 4160, 128) for M in (1, 5, 130)] + [(30528, 146)]
ARG_SHAPES = [(N, M) for N in (64, 192, 320, 4160, 128, 4, 68, 132, 1000) for M in (1, 5, 130)]
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16}


def _labels(M, V, g):
    """Labels at both ends of the vocabulary, on both sides of the first chunk boundary, in the last chunk and ignored
    (-100), then random ones; the M = 1 case gets the last column, the M = 5 case the first five of the list."""
    want = [V - 1, 0, -100, 63, 64, V - 7]
    lab = []
    for c in want:
        if (c == -100 or 0 <= c < V) and c not in lab:
            lab.append(c)
    lab = torch.tensor(lab, dtype=torch.int64)
    rest = torch.randint(0, V, (max(M - len(lab), 0),), generator=g)
    return torch.cat([lab, rest])[:M].to(torch.int32)


@functools.lru_cache(maxsize=None)
def _pool(N, padded):
    """(A [POOL, K], B [N, K], fp32 bias [N], fp64 logits [POOL, N], V).  Rows with a tied row maximum and a chunk
    with a tied chunk maximum come first (a stable reorder of random rows, nothing constructed), so the 1- and 5-row
    cases hold ties as well."""
    g = torch.Generator().manual_seed(1000 + N)
    A = torch.randint(-1, 2, (POOL, K), generator=g).double()
    B = torch.randint(-1, 2, (N, K), generator=g).double()
    V = N - PAD if padded else N
    bias = ((torch.arange(N) % 7) - 3).double()
    if padded:
        B[V:] = 0.0
        bias[V:] = -1e30
    logits = A @ B.t() + bias
    tied = (logits == logits.max(1, keepdim=True).values).sum(1) > 1
    nch = (N + 63) // 64
    lc = torch.full((POOL, nch * 64), float('-inf'), dtype=torch.float64)
    lc[:, :N] = logits
    lc = lc.view(POOL, nch, 64)
    ctied = ((lc == lc.max(2, keepdim=True).values).sum(2) > 1).any(1)
    order = torch.argsort(2 - tied.to(torch.int8) - ctied.to(torch.int8), stable=True)
    return A[order], B, bias.float(), logits[order], V


@functools.lru_cache(maxsize=None)
def _case(N, M, padded):
    """fp64 reference of one (N, M) case: per-chunk {max, sum exp, arg-max, label logit} and the row results."""
    A, B, bias, logits, V = _pool(N, padded)
    A, logits = A[:M], logits[:M]
    nch = (N + 63) // 64
    lab = _labels(M, V, torch.Generator().manual_seed(N + M))
    lp = torch.full((M, nch * 64), float('-inf'), dtype=torch.float64)
    lp[:, :N] = logits
    lc = lp.view(M, nch, 64)
    cmax = lc.max(2).values
    hit = lc == cmax[..., None]
    col = torch.arange(nch * 64).view(1, nch, 64).expand(M, nch, 64)
    carg = torch.where(hit, col, torch.full_like(col, 1 << 40)).min(2).values
    csum = (lc - cmax[..., None]).exp().sum(2)
    onehot = col == lab.view(M, 1, 1).long()
    clab = torch.where(onehot, lc, torch.full_like(lc, float('-inf'))).max(2).values
    rmax = logits.max(1).values
    rhit = logits == rmax[:, None]
    pred = torch.where(rhit, torch.arange(N).expand(M, N), torch.full((M, N), 1 << 40)).min(1).values
    lse = torch.logsumexp(logits, 1)
    lablogit = torch.where(lab >= 0, logits.gather(1, lab.clamp(min=0).long()[:, None])[:, 0],
                           torch.full((M,), float('-inf'), dtype=torch.float64))
    # the tie rule is exercised, not vacuous
    assert (rhit.sum(1) > 1).any(), 'no row with a tied maximum'
    assert (hit.sum(2) > 1).any(), 'no chunk with a tied maximum'
    return dict(A=A, B=B, bias=bias, logits=logits, V=V, nch=nch, lab=lab, cmax=cmax, carg=carg, csum=csum, clab=clab,
                pred=pred, lse=lse, lablogit=lablogit)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _f32(bits):
    return bits.contiguous().view(torch.float32)


def _run_partials(epi, N, M, tile, dtype, padded, width):
    """The epilogue's partial buffer three times -> (spare-column run, production-layout run, its repeat) as int32
    [M + SPARE, ldo, width] on the CPU, and the production-layout buffer on the GPU."""
    c = _case(N, M, padded)
    nch = c['nch']
    A, B = c['A'].to(DEV).to(dtype), c['B'].to(DEV).to(dtype)
    bias, lab = c['bias'].to(DEV), c['lab'].to(DEV)
    runs, dev = [], None
    for ldo in (nch + 1, nch, nch):
        buf = torch.full((M + SPARE, ldo, width), SENTINEL, dtype=torch.int32, device=DEV)
        kw = dict(row_index=lab) if epi == hip.EPI_CE else {}
        hip.gemm_nt(epi, A, B, M, N, K, _f32(buf), bias=bias, ldo=ldo, tile=tile, **kw)
        torch.cuda.synchronize()
        runs.append(buf.cpu())
        dev = buf
    return runs, dev


@functools.lru_cache(maxsize=None)
def _ce_runs(N, M, tile):
    return _run_partials(hip.EPI_CE, N, M, tile, torch.bfloat16, True, 4)


@functools.lru_cache(maxsize=None)
def _argmax_runs(N, M, tile, dt):
    return _run_partials(hip.EPI_ARGMAX, N, M, tile, DTYPES[dt], False, 2)


def _check_guards(runs, M, nch):
    spare_col, prod, again = runs
    for name, buf in (('spare column', spare_col), ('production', prod), ('repeat', again)):
        past = (buf[M:] != SENTINEL).any(2).nonzero()
        assert past.numel() == 0, (f'{name} layout: {past.shape[0]} records of the rows past M were written, first '
                                   f'{buf[M + past[0, 0], past[0, 1]].tolist()} in row M + {past[0, 0].item()}')
        unwritten = int((buf[:M, :nch] == SENTINEL).sum())
        assert unwritten == 0, f'{name} layout: {unwritten} real elements were left unwritten'
    stray = (spare_col[:M, nch:] != SENTINEL).nonzero()
    assert stray.numel() == 0, (f'{stray.shape[0]} stores to chunk index {nch} (past the last chunk), first in row '
                                f'{stray[0, 0].item()}: {spare_col[stray[0, 0], nch].tolist()}')
    assert torch.equal(spare_col[:M, :nch], prod[:M]), 'the partials depend on the leading dimension'
    assert torch.equal(prod, again), 'two runs of the same launch differ'


@pytest.mark.parametrize('tile', [0, 3])
@pytest.mark.parametrize('N,M', CE_SHAPES)
def test_ce_epilogue_guards_and_determinism(N, M, tile):
    _check_guards(_ce_runs(N, M, tile)[0], M, _case(N, M, True)['nch'])


@pytest.mark.parametrize('tile', [0, 3])
@pytest.mark.parametrize('N,M', CE_SHAPES)
def test_ce_epilogue_partials(N, M, tile):
    """max, arg-max and label logit exact; sum exp within 1e-4 relative: the kernel evaluates exp2f((x - max) * log2e)
    in fp32, at |x - max| <= ~180 the rounding of the exponent is ~1.5e-5, the bound about six times that."""
    c = _case(N, M, True)
    for name, buf in zip(('spare column', 'production'), _ce_runs(N, M, tile)[0]):
        real = buf[:M, :c['nch']]
        assert torch.equal(_f32(real[..., 0]).double(), c['cmax']), f'{name}: chunk maximum'
        assert torch.equal(real[..., 2].long(), c['carg']), f'{name}: chunk arg-max (ties -> lowest index)'
        assert torch.equal(_f32(real[..., 3]).double(), c['clab']), f'{name}: label logit (-inf outside the chunk)'
        rel = ((_f32(real[..., 1]).double() - c['csum']).abs() / c['csum']).max().item()
        assert rel <= 1e-4, f'{name}: sum exp off by {rel:.3g} relative'


@pytest.mark.parametrize('tile', [0, 3])
@pytest.mark.parametrize('N,M', CE_SHAPES)
def test_ce_reduce_on_kernel_partials(N, M, tile):
    c = _case(N, M, True)
    part = _f32(_ce_runs(N, M, tile)[1])
    lab = c['lab'].to(DEV)
    for ignore in (-100, 0):
        lse = torch.full((M + 1,), float('nan'), device=DEV)
        loss = torch.full((M + 1,), float('nan'), device=DEV)
        pred = torch.full((M + 1,), -7, dtype=torch.int32, device=DEV)
        hip.ce_reduce(part, c['nch'], lab, ignore, lse, loss, pred, M)
        lse, loss, pred = lse.cpu(), loss.cpu(), pred.cpu()
        assert torch.isnan(lse[M]) and torch.isnan(loss[M]) and pred[M] == -7, 'row M was written'
        assert torch.equal(pred[:M].long(), c['pred']), 'prediction (ties -> lowest index)'
        err = (lse[:M].double() - c['lse']).abs().max().item()
        assert err <= 1e-4, f'lse off by {err:.3g}'
        ignored = c['lab'] == ignore
        assert (loss[:M][ignored] == 0).all(), 'ignored rows must lose exactly 0'
        inside = ~ignored & (c['lab'] >= 0)             # a label outside the vocabulary has no reference loss
        err = (loss[:M].double() - (c['lse'] - c['lablogit']))[inside].abs().max().item() if inside.any() else 0.0
        assert err <= 1e-4, f'row loss off by {err:.3g} (ignore_index {ignore})'


@pytest.mark.parametrize('tile', [0, 3])
@pytest.mark.parametrize('dt', ['bf16', 'f16'])
@pytest.mark.parametrize('N,M', ARG_SHAPES)
def test_argmax_epilogue_guards_and_determinism(N, M, dt, tile):
    _check_guards(_argmax_runs(N, M, tile, dt)[0], M, _case(N, M, False)['nch'])


@pytest.mark.parametrize('tile', [0, 3])
@pytest.mark.parametrize('dt', ['bf16', 'f16'])
@pytest.mark.parametrize('N,M', ARG_SHAPES)
def test_argmax_epilogue_partials_and_reduce(N, M, dt, tile):
    c = _case(N, M, False)
    runs, dev = _argmax_runs(N, M, tile, dt)
    for name, buf in zip(('spare column', 'production'), runs):
        real = buf[:M, :c['nch']]
        assert torch.equal(_f32(real[..., 0]).double(), c['cmax']), f'{name}: chunk maximum'
        assert torch.equal(real[..., 1].long(), c['carg']), f'{name}: chunk arg-max (ties -> lowest index)'
    ids = torch.full((M + 1,), -7, dtype=torch.int64, device=DEV)
    hip.argmax_reduce(_f32(dev), c['nch'], ids, M)
    ids = ids.cpu()
    assert ids[M] == -7, 'row M was written'
    assert torch.equal(ids[:M], c['pred']), 'ids (ties -> lowest index)'


@pytest.mark.parametrize('nchunk', [1, 63, 64, 65, 477])
def test_reduce_kernels_on_hand_built_partials(nchunk):
    """Partials no GEMM produced: integer chunk maxima in [-20, 20] (many chunks share the row maximum), sums in
    [1, 64], and -- from two chunks up -- one chunk per row that holds {-inf, 0, INT_MAX, -inf}, first, last or in the
    middle, which must neither win nor add to the sum."""
    M = 7
    V = nchunk * 64 - PAD
    g = torch.Generator().manual_seed(nchunk)
    lab = _labels(M, V, g)
    mx = torch.randint(-20, 21, (M, nchunk), generator=g).float()
    se = (1 + 63 * torch.rand(M, nchunk, generator=g)).float()
    arg = torch.arange(nchunk)[None] * 64 + torch.randint(0, 64 - PAD, (M, nchunk), generator=g)
    labv = torch.full((M, nchunk), float('-inf'))
    for m in range(M):
        lc = int(lab[m]) // 64 if lab[m] >= 0 else -1
        if lc >= 0:
            labv[m, lc] = mx[m, lc] - float(torch.randint(0, 3, (1,), generator=g))
        if nchunk > 1:
            dead = (0, nchunk - 1, nchunk // 2)[m % 3]
            if dead == lc:
                dead = (dead + 1) % nchunk
            mx[m, dead], se[m, dead], arg[m, dead] = float('-inf'), 0.0, 0x7FFFFFFF
    part = torch.stack([mx, se, torch.zeros_like(mx), labv], 2).contiguous()
    _bits(part)[..., 2] = arg.to(torch.int32)
    gmax = mx.max(1).values
    want_pred = torch.where(mx == gmax[:, None], arg, torch.full_like(arg, 1 << 40)).min(1).values
    assert ((mx == gmax[:, None]).sum(1) > 1).any() or nchunk == 1, 'no row whose maximum is shared between chunks'
    want_lse = gmax.double() + (se.double() * (mx.double() - gmax.double()[:, None]).exp()).sum(1).log()
    want_lab = labv.max(1).values.double()
    pd, labd = part.to(DEV), lab.to(DEV)
    for ignore in (-100, 0):
        lse, loss = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
        pred = torch.empty(M, dtype=torch.int32, device=DEV)
        hip.ce_reduce(pd, nchunk, labd, ignore, lse, loss, pred, M)
        assert torch.equal(pred.cpu().long(), want_pred)
        assert (lse.cpu().double() - want_lse).abs().max().item() <= 1e-4
        ignored = lab == ignore
        assert ignored.any() and (loss.cpu()[ignored] == 0).all()
        inside = ~ignored & (lab >= 0)
        assert (loss.cpu().double() - (want_lse - want_lab))[inside].abs().max().item() <= 1e-4
    pairs = torch.stack([_bits(mx), arg.to(torch.int32)], 2).contiguous()
    ids = torch.empty(M, dtype=torch.int64, device=DEV)
    hip.argmax_reduce(_f32(pairs).to(DEV), nchunk, ids, M)
    assert torch.equal(ids.cpu(), want_pred)


@pytest.mark.parametrize('tile', [0, 3])
@pytest.mark.parametrize('N,M', CE_SHAPES)
def test_ce_bwd_elementwise(N, M, tile):
    """dlogits = (softmax - onehot) * row_scale with the fp64 lse, element by element: one bf16 rounding (2^-8 relative)
    plus 1e-6 * max |row_scale|; padded columns and rows of scale 0 exactly 0; nothing outside [M, N] written."""
    c = _case(N, M, True)
    g = torch.Generator().manual_seed(N * 3 + M)
    rs = (0.5 + torch.rand(M, generator=g)).float()
    rs[c['lab'] == -100] = 0.0
    if M >= 5:
        rs[M // 2] = 0.0
    ldo = N + 8
    out = torch.full((M + 2, ldo), float('nan'), dtype=torch.bfloat16, device=DEV)
    hip.gemm_nt(hip.EPI_CE_BWD, c['A'].to(DEV).bfloat16(), c['B'].to(DEV).bfloat16(), M, N, K, out, bias=c['bias'].to(DEV),
                resid=c['lse'].float().to(DEV), row_scale=rs.to(DEV), row_index=c['lab'].to(DEV), ldo=ldo, tile=tile)
    out = out.cpu()
    assert torch.isnan(out[M:]).all() and torch.isnan(out[:M, N:]).all(), 'an element outside [M, N] was written'
    got = out[:M, :N].double()
    onehot = torch.arange(N)[None] == c['lab'][:, None].long()
    ref = ((c['logits'] - c['lse'][:, None]).exp() - onehot.double()) * rs.double()[:, None]
    over = (got - ref).abs() - (2.0 ** -8 * ref.abs() + 1e-6 * rs.max().item())
    assert over.max().item() <= 0, f'dlogits beyond one bf16 rounding by {over.max().item():.3g}'
    assert (got[:, c['V']:] == 0).all(), 'padded columns must be exactly 0'
    assert (got[rs == 0] == 0).all(), 'rows of scale 0 must be exactly 0'


# ---- LinearCrossEntropyFn end to end --------------------------------------------------------------------------------
# fp32 floor: F.linear + F.cross_entropy in fp32 on the CPU against fp64 at these shapes and operands, measured once:
#   V = 70:    row loss 6.4e-7, mean loss 3.4e-8, dx 5.4e-7, dW 1.6e-7, db 1.1e-7 (gradients relative to their largest element)
#   V = 190:   row loss 1.6e-6, mean loss 2.4e-7, dx 7.9e-7, dW 5.7e-7, db 2.2e-7
#   V = 30522: row loss 1.4e-6, mean loss 1.9e-7, dx 7.8e-7, dW 4.5e-7, db 1.5e-7
# and at the shapes of tests/test_heads_gpu.py row loss 4.7e-7, 1.3e-6, 1.0e-6, 1.5e-7.
# Bounds: eight times the largest floor of each kind (the mean loss is held to the bound of a single row's loss).
LOSS_BOUND = 8 * 1.6e-6
GRAD_FLOOR = 8 * 7.9e-7
E2E_SHAPES = {70: (37, 64), 190: (130, 128), 30522: (146, 64)}


@functools.lru_cache(maxsize=None)
def _e2e_case(V):
    """bf16-exact x [n, d] and W [V, d], fp32 bias; eight labels below 64, three ignored rows."""
    n, d = E2E_SHAPES[V]
    g = torch.Generator().manual_seed(V)
    x = torch.randn(n, d, generator=g).bfloat16().float()
    W = (torch.randn(V, d, generator=g) * 0.25).bfloat16().float()
    b = (torch.randn(V, generator=g) * 0.1).float()
    lab = torch.randint(0, V, (n,), generator=g)
    lab[:8] = torch.arange(8) * 7
    lab[8:11] = -100
    return x, W, b, lab


def _e2e_reference(x, W, b, lab, scale, dtype=torch.float64):
    """(loss, dx, dW, db, |dlogits|) of scale * mean cross-entropy in ``dtype`` on the CPU."""
    x, W = x.to(dtype).requires_grad_(True), W.to(dtype).requires_grad_(True)
    b = None if b is None else b.to(dtype).requires_grad_(True)
    logits = F.linear(x, W, b)
    logits.retain_grad()
    loss = F.cross_entropy(logits, lab, ignore_index=-100)
    (loss * scale).backward()
    return loss.detach(), x.grad, W.grad, None if b is None else b.grad, logits.grad.abs()


def _e2e_check(x, W, b, lab, shadows=None, scale=3.0):
    """Loss within LOSS_BOUND of fp64.  Gradients element by element, relative to the gradient's largest element:
    GRAD_FLOOR plus the bf16 rounding of dlogits (2^-8) times sqrt(reduction length); and, tighter, within what that
    rounding can do to this very element at worst, 2^-8 * sum |dlogits| |other operand|.  -> the loss."""
    from exploremultimodal_amd.derived import Holder
    from exploremultimodal_amd.heads import LinearCrossEntropyFn
    n, V = x.shape[0], W.shape[0]
    xd, Wd = x.to(DEV).requires_grad_(True), W.to(DEV).requires_grad_(True)
    bd = None if b is None else b.to(DEV).requires_grad_(True)
    loss, pred = LinearCrossEntropyFn.apply(xd, Wd, bd, lab.to(DEV), -100, shadows or Holder())
    (loss * scale).backward()
    ref_loss, rdx, rdW, rdb, adl = _e2e_reference(x, W, b, lab, scale)
    err = abs(loss.item() - ref_loss.item())
    assert err <= LOSS_BOUND, f'loss {loss.item():.8g} against {ref_loss.item():.8g}: off by {err:.3g}'
    Vp = (V + 63) // 64 * 64
    cases = [('dx', xd.grad, rdx, Vp, adl @ W.double().abs()), ('dW', Wd.grad, rdW, n, adl.t() @ x.double().abs())]
    if b is not None:
        cases.append(('db', bd.grad, rdb, n, adl.sum(0)))
    for name, got, ref, red, worst in cases:
        got = got.cpu().double()
        assert torch.isfinite(got).all(), name
        top = ref.abs().max().item()
        err = (got - ref).abs()
        rel = err.max().item() / top
        assert rel <= GRAD_FLOOR + 2.0 ** -8 * red ** 0.5, f'{name}: {rel:.3g} of the largest element'
        over = (err - (GRAD_FLOOR * top + 2.0 ** -8 * worst)).max().item()
        assert over <= 0, f'{name}: {over:.3g} beyond the worst case of one bf16 rounding per dlogits element'
    return loss.item(), pred.cpu()


@pytest.mark.parametrize('V', [70, 190, 30522])
def test_linear_cross_entropy_elementwise(V):
    x, W, b, lab = _e2e_case(V)
    assert (lab[:8] < 64).all() and (lab == -100).sum() == 3
    _, pred = _e2e_check(x, W, b, lab)
    logits = x.double() @ W.double().t() + b.double()
    top2 = logits.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert torch.equal(pred.long()[clear], logits.argmax(1)[clear])


@pytest.mark.parametrize('V', [70, 190])
def test_linear_cross_entropy_without_bias(V):
    x, W, _, lab = _e2e_case(V)
    _e2e_check(x, W, None, lab)


@pytest.mark.parametrize('V', [70, 30522])
def test_linear_cross_entropy_all_rows_ignored(V):
    from exploremultimodal_amd.derived import Holder
    from exploremultimodal_amd.heads import LinearCrossEntropyFn
    x, W, b, lab = _e2e_case(V)
    xd, Wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, W, b))
    loss, _ = LinearCrossEntropyFn.apply(xd, Wd, bd, torch.full_like(lab, -100).to(DEV), -100, Holder())
    (loss * 3.0).backward()
    assert loss.item() == 0.0
    for name, t in zip(('dx', 'dW', 'db'), (xd, Wd, bd)):
        assert (t.grad == 0).all(), f'{name} must be exactly 0 (and not NaN) when every row is ignored'


def test_linear_cross_entropy_follows_an_in_place_weight_update():
    """The bf16 shadow copies are keyed by the parameters' version counters: after W.mul_ the same shadow object must
    serve the new weights."""
    from exploremultimodal_amd.derived import Holder
    from exploremultimodal_amd.heads import LinearCrossEntropyFn
    x, W, b, lab = _e2e_case(190)
    sh = Holder()
    Wd, bd = W.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    labd, xd = lab.to(DEV), x.to(DEV)
    first, _ = LinearCrossEntropyFn.apply(xd, Wd, bd, labd, -100, sh)
    with torch.no_grad():
        Wd.mul_(-0.5)               # exact in bf16
        bd.add_(1.0)
        bd[:95].sub_(2.0)
    second, _ = LinearCrossEntropyFn.apply(xd, Wd, bd, labd, -100, sh)
    b2 = b + 1.0
    b2[:95] -= 2.0
    want1 = _e2e_reference(x, W, b, lab, 1.0)[0].item()
    want2 = _e2e_reference(x, W * -0.5, b2, lab, 1.0)[0].item()
    assert abs(want1 - want2) > 100 * LOSS_BOUND
    assert abs(first.item() - want1) <= LOSS_BOUND, (first.item(), want1)
    assert abs(second.item() - want2) <= LOSS_BOUND, (second.item(), want2)
    _e2e_check(x, W * -0.5, b2, lab, shadows=sh)        # the gradients follow too (third call, same shadows, new tensors)
