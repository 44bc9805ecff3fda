"""Task heads of VlmoModule (models/vlmo/heads.py:86-138) with identical parameter names.

The two vocabulary heads -- the MLM decoder tied to the word embedding (768 -> 30 522) and the MIM head
(768 -> 8 192 visual tokens) -- have a fused loss path (``loss_and_pred``): a HIP GEMM whose epilogue keeps per-row
running (max, sum exp, arg-max, label logit) per 64-column chunk, so the [rows, vocabulary] logits never reach HBM, and
a backward that recomputes (softmax - onehot) tile-wise into the bf16 operand of the input- and weight-gradient GEMMs
(VLMO_EPI_CE / VLMO_EPI_CE_BWD, csrc/gemm_common.h).  ``forward`` still returns the logits (reference contract:
`mlm_logits` / `mim_logits` in the output dict); ``config.train.fused_ce`` selects the fused path in the objectives.
The small heads (ITC projection + normalise, 2-way ITM, pooler) are a few MFLOP and stay torch ops.

A Linear -> LayerNorm -> GELU -> Linear classifier runs as ``_mlp_fwd`` / ``_mlp_bwd``: the Linears on the HIP GEMMs,
LayerNorm + GELU on the row kernels of csrc/vqa_head.hip.  ``VQAHeadFn`` is that path for the VQA classifier (hs -> 2hs
-> 3129, vlmo_module.py:85-93) with its binary cross-entropy (objectives.py:317-353) on the row kernel vlmo_vqa_bce.

With ISDA (train.isda_lambda > 0, vlmo_module.py:95-101) the last Linear is ``vqa_last`` and ``ISDAHead`` holds the
per-class feature statistics; a training step with answers runs as ``VQAIsdaHeadFn``: the same path plus the estimator
update and the logit augmentation of heads.py:6-83 on the kernels of csrc/isda.hip, without the reference's [B, vs, 2hs]
tensors.
``isda_update_`` / ``isda_augment`` restate the same arithmetic in torch for features on the CPU."""
import torch
import torch.nn as nn

from . import derived, hip


def _pad64(n):
    return (n + 63) // 64 * 64


# former names of the per-head cache classes: code written against them gets the plain holder.  Construct derived.Holder().
_PaddedShadows = _VQAShadows = derived.Holder


def _pad_vocab_head(weight, bias):
    """bf16 copies of a vocabulary head's weight padded to a multiple of 64 rows (W [Vp, d], W^T [d, Vp]) and its fp32
    bias padded with -1e30 (so padded columns vanish from the soft-max)."""
    V, d = weight.shape
    Vp = _pad64(V)
    w = torch.zeros((Vp, d), dtype=torch.bfloat16, device=weight.device)
    w[:V] = weight.detach()
    wt = w.t().contiguous()
    b = torch.full((Vp,), -1e30, dtype=torch.float32, device=weight.device)
    b[:V] = bias.detach() if bias is not None else 0.0
    return w, wt, b, Vp


class LinearCrossEntropyFn(torch.autograd.Function):
    """mean cross-entropy of ``x @ W^T + b`` against ``labels`` (rows with ``ignore_index`` excluded) and the
    arg-max prediction per row, without materialising the logits (heads.py:86-112 + objectives.py:57-68,571-582).
    ``shadows``: the ``derived.Holder`` that keeps the padded bf16 copies (rebuilt once per optimizer step)."""

    @staticmethod
    def forward(ctx, x, weight, bias, labels, ignore_index, shadows):
        n, d = x.shape
        V = weight.shape[0]
        w, wt, b, Vp = shadows.get('ce', (weight, bias), lambda: _pad_vocab_head(weight, bias))
        xb = x.detach().to(torch.bfloat16).contiguous()
        lab = labels.to(torch.int32).contiguous()
        nch = Vp // 64
        dev = x.device
        part = torch.empty((n, nch, 4), dtype=torch.float32, device=dev)
        hip.gemm_nt(hip.EPI_CE, xb, w, n, Vp, d, part, bias=b, row_index=lab, ldo=nch)
        lse = torch.empty(n, dtype=torch.float32, device=dev)
        rows = torch.empty(n, dtype=torch.float32, device=dev)
        pred = torch.empty(n, dtype=torch.int32, device=dev)
        hip.ce_reduce(part, nch, lab, ignore_index, lse, rows, pred, n)
        valid = labels != ignore_index
        nvalid = valid.sum().clamp(min=1).to(torch.float32)
        ctx.save_for_backward(xb, lab, lse, valid, nvalid, w, wt, b)
        ctx.dims = (n, d, V, Vp, bias is not None)
        ctx.in_dtypes = (x.dtype, weight.dtype, None if bias is None else bias.dtype)
        ctx.mark_non_differentiable(pred)
        return rows.sum() / nvalid, pred

    @staticmethod
    def backward(ctx, dloss, _dpred):
        xb, lab, lse, valid, nvalid, w, wt, b = ctx.saved_tensors
        n, d, V, Vp, has_bias = ctx.dims
        dev = xb.device
        rs = (valid.to(torch.float32) * (dloss.to(torch.float32) / nvalid)).contiguous()
        dlog = torch.empty((n, Vp), dtype=torch.bfloat16, device=dev)
        hip.gemm_nt(hip.EPI_CE_BWD, xb, w, n, Vp, d, dlog, bias=b, resid=lse, row_scale=rs, row_index=lab)
        dx = torch.empty((n, d), dtype=torch.float32, device=dev)
        hip.gemm_nt(hip.EPI_F32, dlog, wt, n, d, Vp, dx)
        dw = torch.zeros((Vp, d), dtype=torch.float32, device=dev)
        hip.gemm_tn(dlog, xb, dw, n, Vp, d)
        db = None
        if has_bias:
            db = torch.zeros(Vp, dtype=torch.float32, device=dev)
            hip.colsum(dlog, db, n, Vp)
            db = db[:V]
        # autograd wants every gradient in its input's dtype: under torch.autocast the activations that reach this head may
        # be half precision (multimodal.py:276-279 runs the module inside autocast)
        xd, wd, bd = ctx.in_dtypes
        return dx.to(xd), dw[:V].to(wd), (db.to(bd) if db is not None else None), None, None, None


def _pad_vqa_head(w1, w2, b2):
    """bf16 copies of the VQA classifier's two weight matrices, zero-padded for the GEMMs (reduction dimensions to a
    multiple of 64, the 3129 answers to 3136), each with its transpose, and the zero-padded fp32 output bias."""
    h2, hs = w1.shape
    vs = w2.shape[0]
    k0, k1, npad = _pad64(hs), _pad64(h2), _pad64(vs)
    dev = w1.device
    w1s = torch.zeros((h2, k0), dtype=torch.bfloat16, device=dev)
    w1s[:, :hs] = w1.detach()
    w1t = torch.zeros((hs, k1), dtype=torch.bfloat16, device=dev)
    w1t[:, :h2] = w1.detach().t()
    w2s = torch.zeros((npad, k1), dtype=torch.bfloat16, device=dev)
    w2s[:vs, :h2] = w2.detach()
    w2t = w2s.t().contiguous()
    b2p = torch.zeros(npad, dtype=torch.float32, device=dev)
    b2p[:vs] = b2.detach()
    return w1s, w1t, w2s, w2t, b2p


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def _mlp_fwd(x, w1, b1, ln_w, ln_b, w2, b2, eps, shadows):
    """Linear(hs, h2) -> LayerNorm -> GELU -> Linear(h2, n) up to the fp32 logits z [B, npad]: x -> bf16 [B, K0] -> GEMM
    (+b1, fp32 out) -> LayerNorm + GELU (bf16 [B, K1]) -> GEMM (+b2).  Pad columns are zero in every operand.  -> (the
    tensors for ``_mlp_bwd``: z, xb, u, h, mean, rstd, gf, bf, w1t, w2t; dims (B, hs, h2, n); the seven input dtypes)."""
    B, hs = x.shape
    h2, n = w1.shape[0], w2.shape[0]
    w1s, w1t, w2s, w2t, b2p = shadows.get('vqa', (w1, w2, b2), lambda: _pad_vqa_head(w1, w2, b2))
    k0, k1, npad = w1s.shape[1], w2s.shape[1], w2s.shape[0]
    dev = x.device
    xb = torch.zeros((B, k0), dtype=torch.bfloat16, device=dev) if k0 != hs else torch.empty((B, k0), dtype=torch.bfloat16, device=dev)
    xb[:, :hs] = x.detach()
    b1f, gf, bf = _f32(b1), _f32(ln_w), _f32(ln_b)
    u = torch.empty((B, h2), dtype=torch.float32, device=dev)
    hip.gemm_nt(hip.EPI_F32, xb, w1s, B, h2, k0, u, bias=b1f)
    h = torch.empty((B, k1), dtype=torch.bfloat16, device=dev)
    mean = torch.empty(B, dtype=torch.float32, device=dev)
    rstd = torch.empty(B, dtype=torch.float32, device=dev)
    hip.ln_gelu_fwd(u, gf, bf, h, mean, rstd, B, h2, eps)
    z = torch.empty((B, npad), dtype=torch.float32, device=dev)
    hip.gemm_nt(hip.EPI_F32, h, w2s, B, npad, k1, z, bias=b2p)
    return ((z, xb, u, h, mean, rstd, gf, bf, w1t, w2t), (B, hs, h2, n),
            tuple(t.dtype for t in (x, w1, b1, ln_w, ln_b, w2, b2)))


def _mlp_bwd(saved, dims, in_dtypes, dz, after_dw2=None):
    """From dz, the bf16 gradient of z (pad columns zero): dh = dz W2, dW2 = dz^T h, db2 = column sums; the LayerNorm +
    GELU backward writes the bf16 operand of dx = du W1, dW1 = du^T x and folds d gamma, d beta, db1 in the same pass.
    ``after_dw2(dw2)`` may add to the fp32 dW2 accumulator [npad, K1] right after its GEMM.  Every reduction runs in a
    fixed order: two runs give the same bits.  -> the seven gradients in their inputs' dtypes."""
    z, xb, u, h, mean, rstd, gf, bf, w1t, w2t = saved
    B, hs, h2, n = dims
    dev = z.device
    npad, k0, k1 = z.shape[1], xb.shape[1], h.shape[1]
    dh = torch.empty((B, k1), dtype=torch.float32, device=dev)
    hip.gemm_nt(hip.EPI_F32, dz, w2t, B, k1, npad, dh)
    dw2 = torch.zeros((npad, k1), dtype=torch.float32, device=dev)
    hip.gemm_tn(dz, h, dw2, B, npad, k1)
    if after_dw2 is not None:
        after_dw2(dw2)
    db2 = torch.zeros(npad, dtype=torch.float32, device=dev)
    for r0 in range(0, B, 1008):      # <= 1008 rows per call: one ordered add per column (reproducible)
        r1 = min(B, r0 + 1008)
        hip.colsum(dz[r0:r1], db2, r1 - r0, npad)
    du = torch.empty((B, k1), dtype=torch.bfloat16, device=dev)
    dg = torch.empty(h2, dtype=torch.float32, device=dev)
    dbeta = torch.empty(h2, dtype=torch.float32, device=dev)
    db1 = torch.empty(h2, dtype=torch.float32, device=dev)
    hip.ln_gelu_bwd(dh, u, gf, bf, mean, rstd, B, h2, dxb=du, dw=dg, db=dbeta, dbias=db1)
    dx = torch.empty((B, hs), dtype=torch.float32, device=dev)
    hip.gemm_nt(hip.EPI_F32, du, w1t, B, hs, k1, dx)
    dw1 = torch.zeros((k1, k0), dtype=torch.float32, device=dev)
    hip.gemm_tn(du, xb, dw1, B, k1, k0)
    xd, w1d, b1d, gd, bd, w2d, b2d = in_dtypes
    return (dx.to(xd), dw1[:h2, :hs].to(w1d), db1.to(b1d), dg.to(gd), dbeta.to(bd), dw2[:n, :h2].to(w2d),
            db2[:n].to(b2d))


def _logits_out(z, n, out_dtype):
    logits = z[:, :n]
    return logits if out_dtype == torch.float32 else logits.to(out_dtype)


def _vqa_loss(z, y, B, vs):
    """-> (sum of the per-row BCE sums / B, arg-max int32 [B], target value at the arg-max [B]); no host read."""
    rows = torch.empty(B, dtype=torch.float32, device=z.device)
    arg = torch.empty(B, dtype=torch.int32, device=z.device)
    score = torch.empty(B, dtype=torch.float32, device=z.device)
    hip.vqa_bce(z, y, B, vs, row_loss=rows, row_arg=arg, row_score=score)
    return rows.sum() / B, arg, score


def _vqa_dz(z, y, B, vs, dlogits, dloss):
    """bf16 [B, npad] gradient of z: (sigmoid(z) - y) * dloss / B when the loss takes part, plus ``dlogits``, the
    gradient of the logits output (e.g. R-Drop's KL term)."""
    dz = torch.empty((B, z.shape[1]), dtype=torch.bfloat16, device=z.device)
    dadd = dlogits.to(torch.float32).contiguous() if dlogits is not None else None
    with_loss = y is not None and dloss is not None
    dscale = dloss.detach().to(torch.float32).reshape(1).contiguous() if with_loss else None
    hip.vqa_bce(z, y if with_loss else None, B, vs, dscale=dscale, alpha=1.0 / B, dadd=dadd, dz=dz)
    return dz


class VQAHeadFn(torch.autograd.Function):
    """``vqa_classifier(x)`` and, when ``targets`` is given, ``BCE-with-logits(logits, targets) * vs`` with the per-row
    arg-max and the target value at it (objectives.py:12-21, 346-351) -> (logits, loss, argmax, score_rows).

    Forward: ``_mlp_fwd`` (fp32 [B, 3136]) -> per-row BCE sum / arg-max / score.  The loss is sum(row sums) / B (= the
    mean over B * vs elements times vs).  Backward: ``_vqa_dz`` -> ``_mlp_bwd``.  Pad columns reach neither the loss,
    the arg-max, the logits nor a gradient.  ``out_dtype``: dtype of the returned logits (the autocast dtype under
    autocast, as the reference's nn.Linear returns); the loss is fp32 and every gradient has its input's dtype."""

    @staticmethod
    def forward(ctx, x, w1, b1, ln_w, ln_b, w2, b2, targets, eps, out_dtype, shadows):
        ctx.set_materialize_grads(False)
        saved, ctx.dims, ctx.in_dtypes = _mlp_fwd(x, w1, b1, ln_w, ln_b, w2, b2, eps, shadows)
        B, _, _, vs = ctx.dims
        z = saved[0]
        loss = arg = score = y = None
        if targets is not None:
            if tuple(targets.shape) != (B, vs):
                raise ValueError(f'vqa targets must be [{B}, {vs}], got {tuple(targets.shape)}')
            y = _f32(targets)
            loss, arg, score = _vqa_loss(z, y, B, vs)
            ctx.mark_non_differentiable(arg, score)
        ctx.save_for_backward(*saved, y)
        return _logits_out(z, vs, out_dtype), loss, arg, score

    @staticmethod
    def backward(ctx, dlogits, dloss, _darg, _dscore):
        *saved, y = ctx.saved_tensors
        B, _, _, vs = ctx.dims
        dz = _vqa_dz(saved[0], y, B, vs, dlogits, dloss)
        return _mlp_bwd(saved, ctx.dims, ctx.in_dtypes, dz) + (None,) * 4


class VQAIsdaHeadFn(torch.autograd.Function):
    """``VQAHeadFn`` with ISDA (heads.py:6-83, objectives.py:325-344) between the last Linear and the loss ->
    (augmented logits, loss, argmax, score_rows).  ``targets`` are required (ISDA runs only on a batch with answers).

    Forward: the head as in VQAHeadFn up to the fp32 logits z [B, npad]; then (1) vlmo_isda_update: the estimator
    buffers ``count`` [vs], ``emean``, ``cov`` [vs, 2hs] (fp32, updated IN PLACE) take this batch's LayerNorm + GELU
    features (recomputed in fp32 from the pre-LayerNorm rows, not the bf16 GEMM operand) and k_n = first arg-max of
    each target row; (2) ck = cov[k] after the update; (3) vlmo_isda_aug_fwd adds 0.5 * ratio * sum_a (W[j] - W[k_n])^2
    ck[n] to z in place (pad columns stay zero); (4) the loss, arg-max and score of vqa_bce on the augmented z.
    Backward: as VQAHeadFn; vlmo_isda_aug_bwd then adds the augmentation's gradient with respect to vqa_last.weight (through
    W[j] and the gathered rows W[k_n]) to the fp32 dW2 accumulator before its cast, from the same bf16 logits gradient
    the GEMMs use.  No gradient reaches the features through the augmentation.  With ratio 0 the augmentation is
    skipped: logits, loss and gradients are VQAHeadFn's bit for bit (the estimator still updates, as upstream)."""

    @staticmethod
    def forward(ctx, x, w1, b1, ln_w, ln_b, w2, b2, targets, eps, out_dtype, shadows, count, emean, cov, ratio):
        ctx.set_materialize_grads(False)
        B, h2, vs = x.shape[0], w1.shape[0], w2.shape[0]
        if targets is None or tuple(targets.shape) != (B, vs):
            raise ValueError(f'ISDA needs vqa targets [{B}, {vs}], got {None if targets is None else tuple(targets.shape)}')
        if tuple(cov.shape) != (vs, h2) or tuple(emean.shape) != (vs, h2) or tuple(count.shape) != (vs,):
            raise ValueError(f'ISDA estimator buffers must be [{vs}], [{vs}, {h2}], [{vs}, {h2}]')
        saved, ctx.dims, ctx.in_dtypes = _mlp_fwd(x, w1, b1, ln_w, ln_b, w2, b2, eps, shadows)
        z, _, u, _, mean, rstd, gf, bf, _, _ = saved
        y = _f32(targets)
        k = torch.empty(B, dtype=torch.int32, device=x.device)
        hip.isda_update(u, y, B, vs, h2, count, emean, cov, k, ln_mean=mean, ln_rstd=rstd, ln_w=gf, ln_b=bf)
        ctx.ratio = float(ratio)
        w2f = ck = None
        if ctx.ratio != 0.0:
            w2f = _f32(w2)
            ck = cov.index_select(0, k)            # cov[k_n] after the update, kept for the backward
            hip.isda_aug_fwd(w2f, k, ck, B, vs, h2, 0.5 * ctx.ratio, z)
        loss, arg, score = _vqa_loss(z, y, B, vs)
        ctx.mark_non_differentiable(arg, score)
        ctx.save_for_backward(*saved, y, w2f, k, ck)
        return _logits_out(z, vs, out_dtype), loss, arg, score

    @staticmethod
    def backward(ctx, dlogits, dloss, _darg, _dscore):
        *saved, y, w2f, k, ck = ctx.saved_tensors
        B, _, h2, vs = ctx.dims
        dz = _vqa_dz(saved[0], y, B, vs, dlogits, dloss)
        aug = (lambda dw2: hip.isda_aug_bwd(dz, w2f, k, ck, B, vs, h2, ctx.ratio, dw2)) if ctx.ratio != 0.0 else None
        return _mlp_bwd(saved, ctx.dims, ctx.in_dtypes, dz, aug) + (None,) * 8


@torch.no_grad()
def isda_update_(count, mean, cov, feats, targets):
    """Estimator update (heads.py:16-50) in place, torch form for CPU features: per class with member rows
    (targets != 0), their mean ``ave`` and population variance ``var``; w = n / (n + count);
    cov <- cov (1 - w) + var w + w (1 - w) (mean - ave)^2, mean <- mean (1 - w) + ave w, count += n.  Only classes with
    members are written."""
    member = targets != 0
    n = member.sum(0)
    cls = n.nonzero().flatten()
    if cls.numel() == 0:
        return
    m = member[:, cls].t().to(feats.dtype)                       # [T, B]
    nc = n[cls].to(feats.dtype)[:, None]
    ave = (m @ feats) / nc
    var = (((feats[None] - ave[:, None]) ** 2) * m[..., None]).sum(1) / nc
    w = nc / (nc + count[cls][:, None])
    mo = mean[cls]
    cov[cls] = cov[cls] * (1 - w) + var * w + w * (1 - w) * (mo - ave) ** 2
    mean[cls] = mo * (1 - w) + ave * w
    count[cls] += n[cls].to(count.dtype)


def isda_augment(logits, weight, cov, k, ratio):
    """logits + 0.5 * ratio * sum_a (W[j, a] - W[k_n, a])^2 cov[k_n, a] (heads.py:55-68), differentiable in ``weight``
    only; the square expanded into three products, so no [B, vs, 2hs] tensor is formed."""
    c = cov[k].detach()                                           # [B, A]
    wk = weight[k]
    quad = (weight * weight) @ c.t() - 2.0 * (weight @ (wk * c).t()) + (wk * wk * c).sum(1)[None]
    return logits + 0.5 * ratio * quad.t()


class EstimatorCV(nn.Module):
    """heads.py:6-14: per-class feature count, mean and diagonal covariance (persistent fp32 buffers)."""

    def __init__(self, hidden_size, class_num):
        super().__init__()
        self.class_num = class_num
        self.register_buffer('count', torch.zeros(class_num))
        self.register_buffer('mean', torch.zeros(class_num, hidden_size))
        self.register_buffer('cov', torch.zeros(class_num, hidden_size))

    def forward(self, features, labels):
        isda_update_(self.count, self.mean, self.cov, features.detach(), labels)


class ISDAHead(nn.Module):
    """heads.py:53-83; ``forward`` is the torch form (CPU features), the GPU step runs VQAIsdaHeadFn."""

    def __init__(self, hidden_size, class_num):
        super().__init__()
        self.estimator = EstimatorCV(hidden_size, class_num)
        self.class_num = class_num

    def forward(self, y, features, fc_weight, target, ratio):
        self.estimator(features, target)
        k = torch.max(target, 1)[1]
        return isda_augment(y, fc_weight, self.estimator.cov, k, ratio)


class BertPredictionHeadTransform(nn.Module):
    """transformers BertPredictionHeadTransform: dense -> GELU -> LayerNorm(eps 1e-12)."""

    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)

    def forward(self, hidden_states):
        return self.LayerNorm(nn.functional.gelu(self.dense(hidden_states)))


class MLMHead(nn.Module):
    """heads.py:86-101 (decoder weight tied to the word embedding, vlmo_module.py:53-55)."""

    def __init__(self, config, weight=None):
        super().__init__()
        self.transform = BertPredictionHeadTransform(config)
        self.decoder = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        self.bias = nn.parameter.Parameter(torch.zeros(config.vocab_size))
        if weight is not None:
            self.decoder.weight = weight

    def forward(self, x):
        return self.decoder(self.transform(x)) + self.bias

    def loss_and_pred(self, x, labels, ignore_index=-100):
        """fused decoder + cross-entropy: (mean loss over rows whose label is not ignore_index, arg-max [n])."""
        return LinearCrossEntropyFn.apply(self.transform(x), self.decoder.weight, self.bias, labels, ignore_index,
                                          derived.of(self))


class MIMHead(nn.Module):
    """heads.py:104-112."""

    def __init__(self, hidden_size, vocab_size):
        super().__init__()
        self.fc = nn.Linear(hidden_size, vocab_size)

    def forward(self, x):
        return self.fc(x)

    def loss_and_pred(self, x, labels, ignore_index=-100):
        return LinearCrossEntropyFn.apply(x, self.fc.weight, self.fc.bias, labels, ignore_index, derived.of(self))


class ITCHead(nn.Module):
    """heads.py:115-127."""

    def __init__(self, hidden_size, out_size):
        super().__init__()
        self.dense = nn.ModuleDict({'v': nn.Linear(hidden_size, out_size), 'l': nn.Linear(hidden_size, out_size)})

    def forward(self, hidden_states, route=None):
        return nn.functional.normalize(self.dense[route](hidden_states), dim=-1)


class ITMHead(nn.Module):
    """heads.py:130-138."""

    def __init__(self, hidden_size):
        super().__init__()
        self.fc = nn.Linear(hidden_size, 2)

    def forward(self, x):
        return self.fc(x)
