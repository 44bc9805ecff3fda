"""Row kernels of the VQA head (csrc/vqa_head.hip) against fp32 torch: LayerNorm + GELU forward / backward at widths
{256, 1536, 2048} (the head of the mini, Base and Large models is 2 * hidden wide) and the per-row BCE / arg-max /
score / logits gradient at 3129 answers; pad columns, reproducibility, argument errors; VQAHeadFn against the torch
modules."""
import pytest
import torch
import torch.nn.functional as F

from exploremultimodal_amd import hip

pytestmark = pytest.mark.gpu
DEV = 'cuda'
VS = 3129


def _ln_inputs(B, d, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, d, device=DEV, generator=g) * 1.5 + 0.3
    w = 1 + 0.1 * torch.randn(d, device=DEV, generator=g)
    b = 0.05 * torch.randn(d, device=DEV, generator=g)
    dh = torch.randn(B, d, device=DEV, generator=g) * 1e-2
    return x, w, b, dh


def _ln_gelu_run(x, w, b, dh, ldh):
    B, d = x.shape
    h = torch.full((B, ldh), 7.0, dtype=torch.bfloat16, device=DEV)           # pads must be overwritten with 0
    mean = torch.empty(B, device=DEV)
    rstd = torch.empty(B, device=DEV)
    hip.ln_gelu_fwd(x, w, b, h, mean, rstd, B, d)
    dx = torch.empty(B, d, device=DEV)
    dxb = torch.full((B, ldh), 7.0, dtype=torch.bfloat16, device=DEV)
    dw, db, dbias = (torch.full((d,), 3.0, device=DEV) for _ in range(3))      # overwritten, not accumulated
    hip.ln_gelu_bwd(dh, x, w, b, mean, rstd, B, d, dx=dx, dxb=dxb, dw=dw, db=db, dbias=dbias)
    torch.cuda.synchronize()
    return h, mean, rstd, dx, dxb, dw, db, dbias


@pytest.mark.parametrize('d', [256, 1536, 2048])
@pytest.mark.parametrize('B', [1, 3, 16, 64, 512])
def test_ln_gelu_matches_fp32_torch(B, d):
    x, w, b, dh = _ln_inputs(B, d, seed=B * 7 + d)
    ldh = d + 64
    h, mean, rstd, dx, dxb, dw, db, dbias = _ln_gelu_run(x, w, b, dh, ldh)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = F.gelu(F.layer_norm(xr, (d,), wr, br, 1e-12))
    y.backward(dh)
    torch.testing.assert_close(mean, x.mean(1), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(rstd, torch.rsqrt(x.var(1, unbiased=False) + 1e-12), atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(h[:, :d].float(), y.detach(), atol=2e-2, rtol=1e-2)          # bf16 output
    assert not h[:, d:].float().any() and not dxb[:, d:].float().any()                   # zero pads
    torch.testing.assert_close(dx, xr.grad, atol=1e-5, rtol=1e-3)
    torch.testing.assert_close(dxb[:, :d].float(), xr.grad, atol=1e-4, rtol=1e-2)
    torch.testing.assert_close(dw, wr.grad, atol=1e-4, rtol=1e-3)
    torch.testing.assert_close(db, br.grad, atol=1e-4, rtol=1e-3)
    torch.testing.assert_close(dbias, xr.grad.sum(0), atol=1e-4, rtol=1e-3)


@pytest.mark.parametrize('d', [256, 2048])
def test_ln_gelu_reproducible(d):
    x, w, b, dh = _ln_inputs(512, d, seed=11)
    r0 = _ln_gelu_run(x, w, b, dh, d)
    r1 = _ln_gelu_run(x, w, b, dh, d)
    for a, c in zip(r0, r1):
        assert torch.equal(a, c)


def test_ln_gelu_rejects_bad_widths():
    for d in (2052, 130):
        x = torch.zeros(4, d, device=DEV)
        w = torch.ones(d, device=DEV)
        h = torch.empty(4, d + 2, dtype=torch.bfloat16, device=DEV)
        m = torch.empty(4, device=DEV)
        with pytest.raises(RuntimeError, match='vlmo_ln_gelu_fwd: need 0 < d <= 2048'):
            hip.ln_gelu_fwd(x, w, w, h, m, m, 4, d)
        with pytest.raises(RuntimeError, match='vlmo_ln_gelu_bwd: need 0 < d <= 2048'):
            hip.ln_gelu_bwd(x, x, w, w, m, m, 4, d, dx=x)


def _bce_inputs(B, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    z = torch.randn(B, 3136, device=DEV, generator=g) * 3
    y = torch.zeros(B, VS, device=DEV)
    for r in range(B):
        k = 1 + r % 10
        cols = torch.randperm(VS, device=DEV, generator=g)[:k]
        y[r, cols] = torch.tensor([0.3, 0.6, 0.9, 1.0], device=DEV)[torch.arange(k, device=DEV) % 4]
    # ties: on every third row the maximum appears twice, at a later and an earlier column -> the earlier one wins
    for r in range(0, B, 3):
        top = z[r, :VS].max() + 1.0
        z[r, 2000] = top
        z[r, 117 + r % 50] = top
        y[r, 117 + r % 50] = 0.9
    return z, y


@pytest.mark.parametrize('B', [1, 3, 16, 64, 512])
def test_vqa_bce_matches_fp32_torch(B):
    z, y = _bce_inputs(B, seed=B)
    rows = torch.empty(B, device=DEV)
    arg = torch.empty(B, dtype=torch.int32, device=DEV)
    score = torch.empty(B, device=DEV)
    hip.vqa_bce(z, y, B, VS, row_loss=rows, row_arg=arg, row_score=score)
    zl = z[:, :VS]
    ref_rows = F.binary_cross_entropy_with_logits(zl.double(), y.double(), reduction='none').sum(1)
    torch.testing.assert_close(rows.double(), ref_rows, atol=1e-3, rtol=1e-5)
    # the loss of the objective: mean over B * vs elements times vs = sum of the row sums / B
    ref_loss = F.binary_cross_entropy_with_logits(zl, y) * VS
    torch.testing.assert_close(rows.sum() / B, ref_loss, atol=1e-3, rtol=1e-5)
    am = zl.argmax(1)
    assert torch.equal(arg.long(), am)
    tie_rows = torch.arange(0, B, 3, device=DEV)
    assert torch.equal(arg[tie_rows].long(), 117 + tie_rows % 50)
    assert torch.equal(score, y[torch.arange(B, device=DEV), am])
    # backward operand: (sigmoid(z) - y) * dloss / B, bf16, pad columns zero; plus an incoming logits gradient
    dscale = torch.tensor([0.75], device=DEV)
    dadd = torch.randn(B, VS, device=DEV) * 1e-3
    dz = torch.full((B, 3136), 5.0, dtype=torch.bfloat16, device=DEV)
    hip.vqa_bce(z, y, B, VS, dscale=dscale, alpha=1.0 / B, dz=dz)
    ref = (torch.sigmoid(zl) - y) * 0.75 / B
    torch.testing.assert_close(dz[:, :VS].float(), ref, atol=1e-6, rtol=1e-2)
    assert not dz[:, VS:].float().any()
    hip.vqa_bce(z, y, B, VS, dscale=dscale, alpha=1.0 / B, dadd=dadd, dz=dz)
    torch.testing.assert_close(dz[:, :VS].float(), ref + dadd, atol=1e-5, rtol=1e-2)
    hip.vqa_bce(z, None, B, VS, dadd=dadd, dz=dz)          # no loss term: the logits gradient alone
    torch.testing.assert_close(dz[:, :VS].float(), dadd, atol=1e-6, rtol=1e-2)
    assert not dz[:, VS:].float().any()


def test_vqa_bce_rejects_bad_arguments():
    z, y = _bce_inputs(2)
    dz = torch.empty(2, 3130, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match='lddz'):
        hip.vqa_bce(z, y, 2, VS, dz=dz)
    with pytest.raises(RuntimeError, match='need targets'):
        hip.vqa_bce(z, None, 2, VS, row_loss=torch.empty(2, device=DEV))


def _head(hs, seed=0):
    g = torch.Generator().manual_seed(seed)
    head = torch.nn.Sequential(torch.nn.Linear(hs, 2 * hs), torch.nn.LayerNorm(2 * hs, eps=1e-12), torch.nn.GELU(),
                               torch.nn.Linear(2 * hs, VS))
    with torch.no_grad():
        for p in head.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() == 2 else 0.02))
        head[1].weight.add_(1.0)
    return head.to(DEV)


def _head_apply(head, x, y, out_dtype=torch.float32):
    from exploremultimodal_amd.derived import Holder
    from exploremultimodal_amd.heads import VQAHeadFn
    fc1, ln, _, fc2 = head
    if not hasattr(head, '_sh'):
        object.__setattr__(head, '_sh', Holder())
    return VQAHeadFn.apply(x, fc1.weight, fc1.bias, ln.weight, ln.bias, fc2.weight, fc2.bias, y, ln.eps, out_dtype,
                           head._sh)


@pytest.mark.parametrize('hs,B', [(128, 3), (768, 64), (1024, 16), (96, 5)])
def test_vqa_head_fn_matches_torch_modules(hs, B):
    """The whole head (bf16 GEMM operands) against the fp32 torch modules; every gradient and its pad handling."""
    head = _head(hs, seed=hs)
    x = torch.randn(B, hs, device=DEV) * 0.5
    y = torch.zeros(B, VS, device=DEV)
    y[torch.arange(B), torch.randint(0, VS, (B,))] = 1.0
    xr = x.clone().requires_grad_(True)
    ref = head(xr)
    ref_loss = F.binary_cross_entropy_with_logits(ref, y) * VS
    ref_loss.backward()
    ref_grads = [p.grad.clone() for p in head.parameters()]
    head.zero_grad(set_to_none=True)
    xh = x.clone().requires_grad_(True)
    logits, loss, arg, score_rows = _head_apply(head, xh, y)
    loss.backward()
    assert logits.shape == (B, VS) and logits.dtype == torch.float32
    torch.testing.assert_close(logits, ref.detach(), atol=3e-2, rtol=3e-2)
    assert abs(loss.item() - ref_loss.item()) <= 2e-2 + 2e-3 * abs(ref_loss.item())
    assert torch.equal(score_rows, y[torch.arange(B), arg.long()])
    for got, want in [(xh.grad, xr.grad)] + list(zip([p.grad for p in head.parameters()], ref_grads)):
        assert got.shape == want.shape and got.dtype == want.dtype
        err = (got - want).norm() / (want.norm() + 1e-12)
        assert err <= 3e-2, (tuple(want.shape), float(err))


def test_vqa_head_fn_reproducible_and_autocast_dtypes():
    head = _head(768)
    x = torch.randn(64, 768, device=DEV)
    y = torch.zeros(64, VS, device=DEV)
    y[:, 5] = 0.6
    runs = []
    for _ in range(2):
        head.zero_grad(set_to_none=True)
        xh = x.clone().requires_grad_(True)
        logits, loss, arg, score = _head_apply(head, xh, y)
        (loss + logits.square().mean()).backward()          # a gradient through the logits output too (R-Drop)
        runs.append([logits.detach(), loss.detach(), arg, score, xh.grad] + [p.grad for p in head.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    for dt in (torch.bfloat16, torch.float16):
        head.zero_grad(set_to_none=True)
        xh = x.to(dt).requires_grad_(True)
        with torch.autocast('cuda', dtype=dt):
            logits, loss, _, _ = _head_apply(head, xh, y, out_dtype=dt)
        assert logits.dtype == dt and loss.dtype == torch.float32
        loss.backward()
        assert xh.grad.dtype == dt and all(p.grad.dtype == torch.float32 for p in head.parameters())
        assert all(torch.isfinite(p.grad).all() for p in head.parameters())
