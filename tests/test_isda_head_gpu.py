"""ISDA kernels (csrc/isda.hip) and heads.VQAIsdaHeadFn on the GPU: the estimator update against an fp64 torch
restatement, the augmentation against fp64 at widths {256, 1536, 2048}, 3129 answers and B in {1, 16, 64, 512}, the
head's gradients against fp32 autograd of the restated formula, reproducibility, argument errors, and ratio 0 against
VQAHeadFn."""
import pytest
import torch
import torch.nn.functional as F

from exploremultimodal_amd import hip
from exploremultimodal_amd.derived import Holder
from exploremultimodal_amd.heads import VQAHeadFn, VQAIsdaHeadFn

pytestmark = pytest.mark.gpu
DEV = 'cuda'
VS = 3129


def _targets(B, V, seed):
    """Soft targets with classes shared by several rows, a few classes hit by many, and rows without an answer."""
    g = torch.Generator().manual_seed(seed)
    y = torch.zeros(B, V)
    for n in range(B):
        if n % 5 == 4:
            continue
        k = int(torch.randint(1, 6, (1,), generator=g))
        cols = torch.randint(0, 40 if n % 2 else V, (k,), generator=g)           # odd rows crowd 40 classes
        y[n, cols] = torch.tensor([0.3, 0.6, 0.9, 1.0])[torch.randint(0, 4, (k,), generator=g)]
    return y.to(DEV)


def _estimator(V, A, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    count = torch.randint(0, 6, (V,), device=DEV, generator=g).float()
    mean = torch.randn(V, A, device=DEV, generator=g) * 0.5
    cov = 0.1 + 0.9 * torch.rand(V, A, device=DEV, generator=g)
    return count, mean, cov


def _update_fp64(count, mean, cov, f, y):
    count, mean, cov, f = (t.double().clone() for t in (count, mean, cov, f))
    member = (y != 0).double()                                            # [B, V]
    n = member.sum(0)
    for c in n.nonzero().flatten().tolist():
        rows = f[member[:, c] > 0]
        ave = rows.mean(0)
        var = ((rows - ave) ** 2).mean(0)
        w = n[c] / (n[c] + count[c])
        cov[c] = cov[c] * (1 - w) + var * w + w * (1 - w) * (mean[c] - ave) ** 2
        mean[c] = mean[c] * (1 - w) + ave * w
        count[c] += n[c]
    return count, mean, cov


def _first_argmax(y):
    m = y.max(1, keepdim=True).values
    idx = torch.arange(y.shape[1], device=y.device).expand_as(y)
    return torch.where(y == m, idx, y.shape[1]).min(1).values


@pytest.mark.parametrize('ln', [False, True])
@pytest.mark.parametrize('B,A', [(1, 256), (16, 1536), (64, 2048), (512, 256)])
def test_isda_update_matches_fp64(B, A, ln):
    g = torch.Generator(device=DEV).manual_seed(B + A)
    u = torch.randn(B, A, device=DEV, generator=g) * 1.3 + 0.2
    y = _targets(B, VS, B * 3 + A)
    count, mean, cov = _estimator(VS, A, 5)
    c0, m0, v0 = count.clone(), mean.clone(), cov.clone()
    k = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    kw = {}
    f = u
    if ln:
        lw = 1 + 0.1 * torch.randn(A, device=DEV, generator=g)
        lb = 0.05 * torch.randn(A, device=DEV, generator=g)
        mu = u.mean(1)
        rs = torch.rsqrt(u.var(1, unbiased=False) + 1e-12)
        kw = dict(ln_mean=mu, ln_rstd=rs, ln_w=lw, ln_b=lb)
        f = F.gelu((u.double() - mu.double()[:, None]) * rs.double()[:, None] * lw.double() + lb.double())
    hip.isda_update(u, y, B, VS, A, count, mean, cov, k, **kw)
    torch.cuda.synchronize()
    rc, rm, rv = _update_fp64(c0, m0, v0, f, y)
    assert torch.equal(k.long(), _first_argmax(y))
    assert (k[(y == 0).all(1)] == 0).all()
    assert torch.equal(count.double(), rc)
    hit = (y != 0).any(0)
    torch.testing.assert_close(mean.double(), rm, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(cov.double(), rv, rtol=1e-4, atol=1e-5)
    # classes without a member row: bitwise unchanged
    assert torch.equal(mean[~hit], m0[~hit]) and torch.equal(cov[~hit], v0[~hit]) and torch.equal(count[~hit], c0[~hit])
    assert hit.sum() > 0 and (B == 1 or ((y != 0).sum(0) >= 2).any())


def _aug_fp64(W, k, ck):
    W, ck = W.double(), ck.double()
    out = torch.empty(k.shape[0], W.shape[0], dtype=torch.float64, device=W.device)
    step = max(1, (1 << 25) // (W.numel()))
    for n0 in range(0, k.shape[0], step):
        kk = k[n0:n0 + step].long()
        d = W[None] - W[kk][:, None]
        out[n0:n0 + step] = (d * d * ck[n0:n0 + step, None]).sum(-1)
    return out


@pytest.mark.parametrize('A', [256, 1536, 2048])
@pytest.mark.parametrize('B', [1, 16, 64, 512])
def test_isda_aug_fwd_matches_fp64(B, A):
    g = torch.Generator(device=DEV).manual_seed(B * 11 + A)
    W = torch.randn(VS, A, device=DEV, generator=g) * 0.02
    k = torch.randint(0, VS, (B,), device=DEV, generator=g).to(torch.int32)
    ck = 0.1 + 0.9 * torch.rand(B, A, device=DEV, generator=g)
    npad = 3136
    z = torch.randn(B, npad, device=DEV, generator=g)
    z[:, VS:] = 0
    z0 = z.clone()
    scale = 1.7
    hip.isda_aug_fwd(W, k, ck, B, VS, A, scale, z)
    torch.cuda.synchronize()
    ref = _aug_fp64(W, k, ck) * scale
    got = (z[:, :VS].double() - z0[:, :VS].double())
    err = (got - ref).abs().max() / ref.abs().max()
    assert err <= 1e-3, float(err)
    assert not z[:, VS:].any()
    # the own-class column gets no augmentation
    assert (got[torch.arange(B), k.long()].abs() <= 1e-5 * ref.abs().max()).all()


def _head_inputs(B, hs, seed, vs=VS):
    g = torch.Generator(device=DEV).manual_seed(seed)
    h2 = 2 * hs
    x = torch.randn(B, hs, device=DEV, generator=g)
    w1 = torch.randn(h2, hs, device=DEV, generator=g) * 0.02
    b1 = torch.randn(h2, device=DEV, generator=g) * 0.02
    lw = 1 + 0.1 * torch.randn(h2, device=DEV, generator=g)
    lb = 0.05 * torch.randn(h2, device=DEV, generator=g)
    w2 = torch.randn(vs, h2, device=DEV, generator=g) * 0.02
    b2 = torch.randn(vs, device=DEV, generator=g) * 0.02
    y = _targets(B, vs, seed + 1)
    return [x, w1, b1, lw, lb, w2, b2], y


def _run_isda(params, y, est, ratio, dlogits_seed=None):
    ps = [p.clone().requires_grad_(True) for p in params]
    count, mean, cov = (t.clone() for t in est)
    logits, loss, arg, score = VQAIsdaHeadFn.apply(*ps, y, 1e-12, torch.float32, Holder(), count, mean, cov, ratio)
    total = loss
    if dlogits_seed is not None:
        gl = torch.Generator(device=DEV).manual_seed(dlogits_seed)
        total = total + (logits * torch.randn(logits.shape, device=DEV, generator=gl) * 1e-3).sum()
    total.backward()
    torch.cuda.synchronize()
    return logits.detach(), loss.detach(), arg, score, [p.grad for p in ps], (count, mean, cov)


def _restated(params, y, est, ratio):
    """fp32 torch of the whole head with ISDA: estimator update, then the augmentation differentiable in W2."""
    ps = [p.clone().requires_grad_(True) for p in params]
    x, w1, b1, lw, lb, w2, b2 = ps
    f = F.gelu(F.layer_norm(F.linear(x, w1, b1), (w1.shape[0],), lw, lb, 1e-12))
    count, mean, cov = (t.clone() for t in est)
    upd = _update_fp64(count, mean, cov, f.detach(), y)
    cov_new = upd[2].float()
    k = _first_argmax(y)
    z = F.linear(f, w2, b2)
    d = w2[None] - w2[k][:, None]
    zaug = z + 0.5 * ratio * (d * d * cov_new[k][:, None]).sum(-1)
    loss = F.binary_cross_entropy_with_logits(zaug, y) * y.shape[1]
    loss.backward()
    return zaug.detach(), loss.detach(), [p.grad for p in ps], upd


@pytest.mark.parametrize('hs', [128, 768])
def test_isda_head_gradients_match_fp32_autograd(hs):
    B = 16
    params, y = _head_inputs(B, hs, seed=hs)
    est = _estimator(VS, 2 * hs, 9)
    ratio = 3.75
    logits, loss, _, _, grads, (count, mean, cov) = _run_isda(params, y, est, ratio)
    rl, rloss, rgrads, (rc, rm, rv) = _restated(params, y, est, ratio)
    assert float((logits - rl).abs().max()) <= 5e-2 + 1e-2 * float(rl.abs().max())
    assert abs(float(loss) - float(rloss)) <= 2e-2 * abs(float(rloss)) + 1e-3
    assert torch.equal(count.double(), rc)
    torch.testing.assert_close(mean.double(), rm, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(cov.double(), rv, rtol=2e-2, atol=2e-2)
    names = ['x', 'w1', 'b1', 'ln_w', 'ln_b', 'w2', 'b2']
    for n, gg, rg in zip(names, grads, rgrads):
        rel = float((gg - rg).norm() / rg.norm())
        assert rel <= 3e-2, (n, rel)
    # the ISDA part of dW2 on its own: gradient with ratio minus gradient at ratio 0
    _, _, _, _, g0, _ = _run_isda(params, y, est, 0.0)
    _, _, rg0, _ = _restated(params, y, est, 0.0)
    d_isda, r_isda = grads[5] - g0[5], rgrads[5] - rg0[5]
    assert float(r_isda.norm()) > 0.05 * float(rgrads[5].norm())
    assert float((d_isda - r_isda).norm() / r_isda.norm()) <= 3e-2


def test_isda_head_is_reproducible():
    params, y = _head_inputs(64, 768, seed=3)
    est = _estimator(VS, 1536, 4)
    a = _run_isda(params, y, est, 2.0, dlogits_seed=1)
    b = _run_isda(params, y, est, 2.0, dlogits_seed=1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for ga, gb in zip(a[4], b[4]):
        assert torch.equal(ga, gb)
    for ta, tb in zip(a[5], b[5]):
        assert torch.equal(ta, tb)


def test_isda_ratio_zero_is_the_plain_head():
    params, y = _head_inputs(16, 128, seed=8)
    est = _estimator(VS, 256, 2)
    logits, loss, arg, score, grads, (count, _, _) = _run_isda(params, y, est, 0.0, dlogits_seed=5)
    ps = [p.clone().requires_grad_(True) for p in params]
    l2, loss2, arg2, score2 = VQAHeadFn.apply(*ps, y, 1e-12, torch.float32, Holder())
    gl = torch.Generator(device=DEV).manual_seed(5)
    (loss2 + (l2 * torch.randn(l2.shape, device=DEV, generator=gl) * 1e-3).sum()).backward()
    assert torch.equal(logits, l2.detach()) and torch.equal(loss, loss2.detach())
    assert torch.equal(arg, arg2) and torch.equal(score, score2)
    for ga, p in zip(grads, ps):
        assert torch.equal(ga, p.grad)
    assert not torch.equal(count, est[0])            # the estimator still learns at ratio 0


def test_isda_bad_arguments():
    B, A = 4, 256
    W = torch.zeros(VS, A, device=DEV)
    k = torch.zeros(B, dtype=torch.int32, device=DEV)
    ck = torch.zeros(B, A, device=DEV)
    z = torch.zeros(B, 3136, device=DEV)
    with pytest.raises(RuntimeError, match='A <= 2048'):
        Wb = torch.zeros(VS, 2112, device=DEV)
        hip.isda_aug_fwd(Wb, k, torch.zeros(B, 2112, device=DEV), B, VS, 2112, 1.0, z)
    with pytest.raises(RuntimeError, match='A % 4'):
        hip.isda_aug_fwd(W, k, ck, B, VS, 254, 1.0, z)
    with pytest.raises(RuntimeError, match='vlmo_isda_aug_bwd'):
        hip.isda_aug_bwd(torch.zeros(B, 3136, dtype=torch.bfloat16, device=DEV), W, k, ck, B, VS, A, 1.0,
                         torch.zeros(VS, 128, device=DEV))                 # dW narrower than A
    with pytest.raises(ValueError, match='bf16'):
        hip.isda_aug_bwd(torch.zeros(B, 3136, device=DEV), W, k, ck, B, VS, A, 1.0, torch.zeros(VS, A, device=DEV))
    count, mean, cov = _estimator(VS, A, 0)
    y = torch.zeros(B, VS, device=DEV)
    with pytest.raises(RuntimeError, match='vlmo_isda_update'):
        hip.isda_update(torch.zeros(B, A, device=DEV), y, B, VS, 0, count, mean, cov, k)
    with pytest.raises(ValueError, match='contiguous fp32'):
        hip.isda_update(torch.zeros(B, A, device=DEV), y, B, VS, A, count, mean.half(), cov, k)
    params, yy = _head_inputs(B, 256, seed=1)
    with pytest.raises(ValueError, match='targets'):
        VQAIsdaHeadFn.apply(*params, yy[:, :100], 1e-12, torch.float32, Holder(), count, mean, cov, 1.0)
    with pytest.raises(ValueError, match='buffers'):
        VQAIsdaHeadFn.apply(*params, yy, 1e-12, torch.float32, Holder(), count, mean, cov, 1.0)   # buffers 256 wide, head 512
