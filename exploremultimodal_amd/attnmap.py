"""Attention maps: the soft-max probabilities the blocks compute, materialised for inspection.

The reference's ``Attention.forward`` / ``Block.forward`` return ``(x, attn)`` with ``attn`` the [B, heads, N, N]
soft-max matrix (vlmo.py:88-98, 187-197).  The fused attention kernels of this engine never form it; this module does, on
request, with one HIP kernel (``vlmo_attn_probs``) next to the training path: nothing here changes what a forward or a
backward pass computes.

Definition (one sequence, one head; q, k the engine's bf16 rows, fp32 accumulation):

    P = softmax(q k^T * scale + keymask(-inf), dim=-1)

with these zero rules:
  * a masked key is exactly 0;
  * a padded QUERY position is a row like any other (only keys are masked, as in the reference);
  * key columns and query rows past a sequence's own length (a sequence shorter than ``seq_len``) are 0;
  * a row whose keys are ALL masked is 0 -- the reference's soft-max gives NaN there.

The maps are PRE-dropout (the reference returns the post-dropout tensor in training mode; the model-level entry points
refuse training mode) and carry no autograd graph.

Memory: 4 * seq_len^2 bytes per sequence and head -- 209 MB per layer for VLMo-Base at 64 pairs (261 tokens), 4 * 965^2 *
heads * B bytes at 480 px.  ``queries=(q0, nq)`` (a window of query rows) and ``head_mean=True`` (the mean over heads)
exist to cut that down.

Gradient-weighted maps (Grad-CAM on ``attn``, ``vlmo_attn_gradcam``).  With P taken as a free variable of ctx = P v, the
gradient of a score with respect to it is, per head,

    G[i, j] = sum_c dctx[row_i, 64 h + c] * v[row_j, 64 h + c]          (bf16 products, fp32 accumulation)

with dctx the bf16 [M, d] gradient of the attention context on the packed rows (head-major like ctx) -- what the
reference obtains with a hook and ``retain_grad()`` on the ``attn`` tensor.  kind 'grad' gives G, 'attn_grad' P * G,
'cam' (the default) P * max(G, 0).  The zero rules above hold for every kind, 'grad' included; ``head_mean`` is the mean
over heads of the per-head output (of the products, not the product of the means).  Shapes, windows and memory are those
of the maps.

Relevance over the depth (Chefer et al.'s propagation, attention rollout; ``vlmo_relevance_step``): the head-mean maps of
the layers multiplied into relevance rows from the top layer down -- defined where the relevance_* functions begin.
"""
import torch

from . import engine, hip

HEAD_DIM = 64
MAX_LEN = 1024


def _resolve(qkv, seg, num_seq, seq_len, heads, keymask, scale, queries):
    """Validate the arguments of attention_probs / attention_probs_reference -> (scale, q0, nq)."""
    if heads < 1 or num_seq < 1:
        raise ValueError(f'need heads >= 1 and num_seq >= 1 (heads={heads}, num_seq={num_seq})')
    if qkv.dim() != 2 or qkv.shape[1] != 3 * HEAD_DIM * heads:
        raise ValueError(f'qkv must be [M, {3 * HEAD_DIM * heads}] (q | k | v, head_dim {HEAD_DIM}), got {tuple(qkv.shape)}')
    if not 1 <= seq_len <= MAX_LEN:
        raise ValueError(f'seq_len must be in [1, {MAX_LEN}], got {seq_len}')
    if seg.dim() != 2 or seg.shape[1] != 4 or seg.shape[0] < num_seq:
        raise ValueError(f'seg must be [>= {num_seq}, 4] (rowA, lenA, rowB, lenB), got {tuple(seg.shape)}')
    if keymask is not None and (keymask.dim() != 1 or keymask.shape[0] != qkv.shape[0]):
        raise ValueError(f'keymask must be [{qkv.shape[0]}], got {tuple(keymask.shape)}')
    q0, nq = (0, seq_len) if queries is None else (int(queries[0]), int(queries[1]))
    if q0 < 0 or nq < 1 or q0 + nq > seq_len:
        raise ValueError(f'queries=({q0}, {nq}) is not a window of [0, {seq_len})')
    return (HEAD_DIM ** -0.5 if scale is None else float(scale)), q0, nq


KINDS = ('cam', 'attn_grad', 'grad')


def _resolve_gradcam(qkv, dctx, heads, kind):
    """The arguments attention_gradcam / attention_gradcam_reference have on top of _resolve's."""
    if kind not in KINDS:
        raise ValueError(f'kind must be one of {KINDS}, got {kind!r}')
    if dctx.dim() != 2 or tuple(dctx.shape) != (qkv.shape[0], HEAD_DIM * heads):
        raise ValueError(f'dctx must be [{qkv.shape[0]}, {HEAD_DIM * heads}] (the rows of qkv, head-major), '
                         f'got {tuple(dctx.shape)}')


def _restate(qkv, dctx, seg, num_seq, seq_len, heads, keymask, scale, q0, nq, head_mean, kind, dtype):
    """The definitions of the module docstring in plain torch: P when ``kind`` is None, else the gradient-weighted map."""
    d = HEAD_DIM * heads
    out = torch.zeros((num_seq, heads, nq, seq_len), dtype=dtype, device=qkv.device)
    for s, (row_a, len_a, row_b, len_b) in enumerate(seg[:num_seq].tolist()):
        len_a = min(max(len_a, 0), seq_len)
        len_b = min(max(len_b, 0), seq_len - len_a)
        n = len_a + len_b
        rows = torch.cat([torch.arange(row_a, row_a + len_a), torch.arange(row_b, row_b + len_b)]).to(qkv.device)
        hi = min(q0 + nq, n)
        if hi <= q0:
            continue
        x = qkv[rows].to(dtype)
        q = x[q0:hi, :d].reshape(hi - q0, heads, HEAD_DIM).transpose(0, 1)
        k = x[:, d:2 * d].reshape(n, heads, HEAD_DIM).transpose(0, 1)
        scores = (q @ k.transpose(-2, -1)) * scale
        valid = None
        if keymask is not None:
            valid = keymask[rows] != 0
            if not bool(valid.any()):
                continue                        # every key masked: zeros (the reference has NaN)
            scores = scores.masked_fill(~valid[None, None, :], float('-inf'))
        val = scores.softmax(dim=-1)
        if kind is not None:
            v = x[:, 2 * d:].reshape(n, heads, HEAD_DIM).transpose(0, 1)
            g = dctx[rows[q0:hi]].to(dtype).reshape(hi - q0, heads, HEAD_DIM).transpose(0, 1)
            G = g @ v.transpose(-2, -1)
            if valid is not None:
                G = G.masked_fill(~valid[None, None, :], 0.0)
            val = G if kind == 'grad' else val * (G.clamp_min(0.0) if kind == 'cam' else G)
        out[s, :, :hi - q0, :n] = val
    return out.mean(dim=1, keepdim=True) if head_mean else out


def attention_probs_reference(qkv, seg, num_seq, seq_len, heads, keymask=None, scale=None, queries=None,
                              head_mean=False, dtype=torch.float32):
    """The definition above in plain torch (any device), computed in ``dtype`` (float32 or float64) from the values of
    ``qkv`` as they are.  Returns [num_seq, 1 if head_mean else heads, nq, seq_len]."""
    scale, q0, nq = _resolve(qkv, seg, num_seq, seq_len, heads, keymask, scale, queries)
    return _restate(qkv, None, seg, num_seq, seq_len, heads, keymask, scale, q0, nq, head_mean, None, dtype)


def attention_gradcam_reference(qkv, dctx, seg, num_seq, seq_len, heads, keymask=None, scale=None, queries=None,
                                head_mean=False, kind='cam', dtype=torch.float32):
    """The gradient-weighted map of the module docstring in plain torch (any device), computed in ``dtype`` (float32 or
    float64) from the values of ``qkv`` and ``dctx`` as they are -> [num_seq, 1 if head_mean else heads, nq, seq_len]."""
    scale, q0, nq = _resolve(qkv, seg, num_seq, seq_len, heads, keymask, scale, queries)
    _resolve_gradcam(qkv, dctx, heads, kind)
    return _restate(qkv, dctx, seg, num_seq, seq_len, heads, keymask, scale, q0, nq, head_mean, kind, dtype)


def attention_probs(qkv, seg, num_seq, seq_len, heads, keymask=None, scale=None, queries=None, head_mean=False):
    """P of every sequence of ``seg`` over the packed rows of ``qkv`` [M, 3 * 64 * heads] -> fp32
    [num_seq, 1 if head_mean else heads, nq, seq_len].

    seg int32 [num_seq, 4] = (rowA, lenA, rowB, lenB): sequence s = rows [rowA, rowA + lenA) ++ [rowB, rowB + lenB), as
    for the fused attention; seq_len >= every sequence's length, <= 1024.  keymask int32 [M] (0 = masked key) or None.
    queries = (q0, nq): only query rows [q0, q0 + nq); default all.  scale defaults to 64 ** -0.5.
    Device tensors (bf16 qkv) take the HIP kernel; CPU tensors take attention_probs_reference in fp32."""
    scale, q0, nq = _resolve(qkv, seg, num_seq, seq_len, heads, keymask, scale, queries)
    if not qkv.is_cuda:
        return attention_probs_reference(qkv, seg, num_seq, seq_len, heads, keymask, scale, (q0, nq), head_mean)
    if qkv.dtype != torch.bfloat16 or not qkv.is_contiguous():
        raise ValueError('device qkv must be a contiguous bf16 matrix (the engine\'s qkv rows)')
    seg = seg.to(device=qkv.device, dtype=torch.int32).contiguous()
    if keymask is not None:
        keymask = keymask.to(device=qkv.device, dtype=torch.int32).contiguous()
    probs = torch.empty((num_seq, 1 if head_mean else heads, nq, seq_len), dtype=torch.float32, device=qkv.device)
    hip.attn_probs(qkv, seg, num_seq, keymask, probs, heads, HEAD_DIM * heads, seq_len, q0, nq, head_mean, scale)
    return probs


def attention_gradcam(qkv, dctx, seg, num_seq, seq_len, heads, keymask=None, scale=None, queries=None, head_mean=False,
                      kind='cam'):
    """The gradient-weighted map of every sequence of ``seg``: 'cam' P * max(G, 0), 'attn_grad' P * G or 'grad' G with
    G = dctx v^T per head -> fp32 [num_seq, 1 if head_mean else heads, nq, seq_len].  dctx [M, 64 * heads]: the gradient
    of the attention context on the rows of ``qkv``; everything else as attention_probs.
    Device tensors (contiguous bf16 qkv and dctx) take the HIP kernel; CPU tensors take attention_gradcam_reference."""
    scale, q0, nq = _resolve(qkv, seg, num_seq, seq_len, heads, keymask, scale, queries)
    _resolve_gradcam(qkv, dctx, heads, kind)
    if not qkv.is_cuda:
        return attention_gradcam_reference(qkv, dctx, seg, num_seq, seq_len, heads, keymask, scale, (q0, nq), head_mean,
                                           kind)
    if qkv.dtype != torch.bfloat16 or not qkv.is_contiguous():
        raise ValueError('device qkv must be a contiguous bf16 matrix (the engine\'s qkv rows)')
    if dctx.device != qkv.device or dctx.dtype != torch.bfloat16 or not dctx.is_contiguous():
        raise ValueError('device dctx must be a contiguous bf16 matrix on the device of qkv (the engine\'s dctx rows)')
    seg = seg.to(device=qkv.device, dtype=torch.int32).contiguous()
    if keymask is not None:
        keymask = keymask.to(device=qkv.device, dtype=torch.int32).contiguous()
    out = torch.empty((num_seq, 1 if head_mean else heads, nq, seq_len), dtype=torch.float32, device=qkv.device)
    hip.attn_gradcam(qkv, dctx, seg, num_seq, keymask, out, heads, HEAD_DIM * heads, seq_len, q0, nq, kind, head_mean, scale)
    return out


def text_to_image_heatmaps(cam, T, grid):
    """Text-token rows against image-patch columns of a FUSED-layer map [B, heads | 1, nq, T + 1 + grid^2] (text first,
    then the image CLS, then the patches row by row) -> [B, heads | 1, T, grid, grid]: one heat map over the image per
    text token.  The map must hold the query rows [0, T) first (the full map, or queries=(0, T))."""
    if cam.dim() != 4 or cam.shape[2] < T or cam.shape[3] != T + 1 + grid * grid:
        raise ValueError(f'need a fused-layer map [B, heads | 1, >= {T}, {T + 1 + grid * grid}], got {tuple(cam.shape)}')
    return cam[:, :, :T, T + 1:].reshape(cam.shape[0], cam.shape[1], T, grid, grid)


# ---- model plumbing: the qkv rows of a block, by the launches the stack itself uses -----------------------------------

@torch.no_grad()
def block_qkv(block, x, shadows):
    """bf16 qkv [M, 3d] of ``block`` for the packed fp32 activations x [M, d] that enter it: norm1 to bf16 (vlmo_ln_fwd),
    then the qkv GEMM with the bias q_bias | 0 | v_bias in its epilogue (vlmo_gemm_nt) -- what vlmo_stack_fwd runs."""
    M, d = x.shape
    a = block.attn
    qb, vb = (a.q_bias, a.v_bias) if a.q_bias is not None else (a._zero_bias, a._zero_bias)
    y1 = torch.empty((M, d), dtype=torch.bfloat16, device=x.device)
    mean, rstd = torch.empty(M, device=x.device), torch.empty(M, device=x.device)
    hip.ln_fwd(x, block.norm1.weight.detach(), block.norm1.bias.detach(), y1, mean, rstd, None, M, d, block.norm1.eps)
    qkv = torch.empty((M, 3 * d), dtype=torch.bfloat16, device=x.device)
    hip.gemm_nt(hip.EPI_BIAS, y1, shadows.get(a.qkv.weight, need_t=False)[0], M, 3 * d, d, qkv,
                tile=engine.DEFAULT_TILE, bias=shadows.qkv_bias(qb, vb))
    return qkv


def plan_kinds(plan, fused):
    """The sequence kinds of a block call under ``plan``: [(name or None, seg, seq_len)].  Below the fusion layer of an
    image-text pass the reference calls the block once per modality (vlmo.py:402-404): two kinds, 'txt' and 'img'."""
    if plan.T and plan.P:
        if fused:
            return [(None, plan.seg_vl, plan.T + plan.P)]
        return [('txt', plan.seg_txt, plan.T), ('img', plan.seg_img, plan.P)]
    return [(None, plan.seg_txt, plan.T)] if plan.T else [(None, plan.seg_img, plan.P)]


@torch.no_grad()
def block_maps(block, x, plan, fused, shadows, queries=None, head_mean=False):
    """The attention map(s) of one block call on packed activations x: a tensor [B, heads | 1, nq, N], or
    {'txt': ..., 'img': ...} when the call has two kinds of sequence."""
    kinds = plan_kinds(plan, fused)
    if queries is not None and len(kinds) > 1:
        raise ValueError('queries needs a single kind of sequence; this layer attends text and image separately')
    qkv = block_qkv(block, x, shadows)
    maps = {name: attention_probs(qkv, seg, plan.B, n, block.num_heads, plan.keymask, block.attn.scale, queries, head_mean)
            for name, seg, n in kinds}
    return maps[None] if len(kinds) == 1 else maps


def gradcam_capture(block, store, key, queries=None, head_mean=False, kind='cam'):
    """The engine.BlockMeta.capture callback of one block call: launches vlmo_attn_gradcam on the block's saved qkv rows
    and its dctx, straight from the engine's buffers on the backward's stream, and files the map(s) as store[key] -- a
    tensor [B, heads | 1, nq, N], or {'txt': ..., 'img': ...} when the call has two kinds of sequence."""
    def capture(qkv, dctx, plan, fused):
        kinds = plan_kinds(plan, fused)
        maps = {name: attention_gradcam(qkv, dctx, seg, plan.B, n, block.num_heads, plan.keymask, block.attn.scale,
                                        queries, head_mean, kind) for name, seg, n in kinds}
        store[key] = maps[None] if len(kinds) == 1 else maps
    return capture


# ---- relevance over the depth: Chefer et al.'s propagation and attention rollout (vlmo_relevance_step) ------------------
#
# With Abar_l the [B, N, N] head-mean map of layer l in the token order of forward_features (text first) -- 'gradcam':
# mean_h P_h * max(G_h, 0), (alpha, beta) = (1, 1); 'rollout': mean_h P_h, (alpha, beta) = (0.5, 0.5); below the fusion layer
# of an image-text pass blockdiag(Abar_txt [T, T], Abar_img [P, P]) -- the relevance is
#
#     R = prod_{l = L-1 .. 0} (alpha I + beta Abar_l)          (top layer leftmost)
#
# which is R <- alpha R + beta Abar_l R from layer 0 upward, starting at I.  Only rows are wanted, so rows are carried from
# the top layer downward: X = I[q0 : q0 + nq], then X <- alpha X + beta X @ Abar_l for l = L-1 .. 0 (relevance_step).  A
# layer that is left out contributes the factor I.  Nothing is normalised; every quantity is >= 0.  Zero rules, from those of
# the maps: a masked key is a zero column of every Abar_l, so its relevance column holds the identity part only (alpha^L on
# its own row, 0 elsewhere); a query row whose keys are all masked propagates alpha X only.

METHODS = {'gradcam': (1.0, 1.0), 'rollout': (0.5, 0.5)}


def method_weights(method):
    """(alpha, beta) of ``method``; ValueError for an unknown one."""
    if method not in METHODS:
        raise ValueError(f'method must be one of {tuple(METHODS)}, got {method!r}')
    return METHODS[method]


def resolve_rows(queries, N):
    """queries=(q0, nq) over the N concatenated tokens (None: all of them) -> (q0, nq); ValueError outside [0, N]."""
    q0, nq = (0, N) if queries is None else (int(queries[0]), int(queries[1]))
    if q0 < 0 or nq < 1 or q0 + nq > N:
        raise ValueError(f'queries=({q0}, {nq}) is not a window of the {N} tokens')
    return q0, nq


def check_layers(layers, L):
    """The ``layers`` argument of the relevance entry points -> ascending list (None: all); ValueError for an index outside
    [0, L) and for an unsorted or repeated list (the product has an order: a list that states another one is refused)."""
    if layers is None:
        return list(range(L))
    layers = [int(i) for i in layers]
    if any(i < 0 or i >= L for i in layers):
        raise ValueError(f'layers must be block indices in [0, {L}), got {layers}')
    if any(b <= a for a, b in zip(layers, layers[1:])):
        raise ValueError(f'layers must be strictly ascending, got {layers}')
    return layers


def _square(m, what):
    """A head-mean map [B, 1, n, n] or [B, n, n] -> [B, n, n]."""
    if m.dim() == 4 and m.shape[1] == 1:
        m = m[:, 0]
    if m.dim() != 3 or m.shape[1] != m.shape[2]:
        raise ValueError(f'{what} must be a head-mean map of every query row, [B, 1, n, n] or [B, n, n], got '
                         f'{tuple(m.shape)}')
    return m


def _blocks(m, N, T):
    """A layer's map or {'txt', 'img'} dict -> [(c0, Abar [B, n, n])], the diagonal blocks that tile the N columns."""
    if isinstance(m, dict):
        if set(m) != {'txt', 'img'}:
            raise ValueError(f"a per-modality layer must be {{'txt': ..., 'img': ...}}, got keys {sorted(m)}")
        txt, img = _square(m['txt'], "the 'txt' map"), _square(m['img'], "the 'img' map")
        if txt.shape[1] + img.shape[1] != N or (T is not None and txt.shape[1] != T) or txt.shape[0] != img.shape[0]:
            raise ValueError(f'per-modality maps of {txt.shape[1]} + {img.shape[1]} tokens do not tile N={N} (T={T})')
        return [(0, txt), (txt.shape[1], img)]
    m = _square(m, 'a map')
    if m.shape[1] != N:
        raise ValueError(f'a map of {m.shape[1]} tokens where N={N}')
    return [(0, m)]


def relevance_step(A, x, c0=0, alpha=1.0, beta=1.0):
    """One step of the row form: a NEW tensor y [S, nq, width] with
    y[s, r, c0 + j] = alpha x[s, r, c0 + j] + beta sum_{k < n} x[s, r, c0 + k] A[s, k, j] for A [S, n, n], and the columns
    outside [c0, c0 + n) copied from x.  Device fp32 contiguous tensors take the HIP kernel (vlmo_relevance_step); CPU
    tensors take this restatement in their own dtype."""
    if A.dim() != 3 or A.shape[1] != A.shape[2] or x.dim() != 3 or x.shape[0] != A.shape[0]:
        raise ValueError(f'need A [S, n, n] and x [S, nq, width], got {tuple(A.shape)} and {tuple(x.shape)}')
    n, width = A.shape[1], x.shape[2]
    c0 = int(c0)
    if c0 < 0 or c0 + n > width:
        raise ValueError(f'columns [{c0}, {c0 + n}) are not inside the width {width}')
    if not x.is_cuda:
        y = x.clone()
        y[:, :, c0:c0 + n] = alpha * x[:, :, c0:c0 + n] + beta * (x[:, :, c0:c0 + n] @ A.to(x.dtype))
        return y
    if A.dtype != torch.float32 or x.dtype != torch.float32 or not A.is_contiguous() or not x.is_contiguous():
        raise ValueError('device A and x must be contiguous fp32 tensors')
    y = torch.empty_like(x) if n == width else x.clone()
    hip.relevance_step(A, x, y, c0, alpha, beta)
    return y


def relevance_propagate(X, m, T, alpha, beta):
    """X <- alpha X + beta X @ Abar for the map (or per-modality dict) ``m`` of one layer -> a new [B, nq, N] tensor.  A
    per-modality layer is one kernel call per diagonal block into the same output: the two column ranges tile the width."""
    blocks = _blocks(m, X.shape[2], T)
    if not X.is_cuda:
        for c0, A in blocks:
            X = relevance_step(A, X, c0, alpha, beta)
        return X
    Y = torch.empty_like(X)
    for c0, A in blocks:
        hip.relevance_step(A.contiguous(), X, Y, c0, alpha, beta)
    return Y


def relevance_rows(B, N, q0, nq, device, dtype=torch.float32):
    """I[q0 : q0 + nq, :] for every sample -> [B, nq, N]: where the row form starts."""
    X = torch.zeros((B, nq, N), dtype=dtype, device=device)
    X[:, torch.arange(nq, device=device), torch.arange(q0, q0 + nq, device=device)] = 1.0
    return X


def relevance_reference(maps, N, T=None, queries=None, method='gradcam', dtype=torch.float32):
    """The definition above in plain torch (any device), computed in ``dtype`` (float32 or float64): ``maps`` is
    {layer: map-or-dict} as attention_maps / attention_gradcam return it with head_mean=True and every query row; layers
    that are not in it contribute the factor I.  R <- alpha R + beta Abar_l R over the whole [N, N] matrix from the lowest
    layer upward, then rows [q0, q0 + nq) -> [B, nq, N].  T (the text length) is needed only to check per-modality maps."""
    alpha, beta = method_weights(method)
    q0, nq = resolve_rows(queries, N)
    if not maps:
        raise ValueError('maps is empty: pass at least one layer')
    R = None
    for i in sorted(maps):
        blocks = _blocks(maps[i], N, T)
        if R is None:
            B, dev = blocks[0][1].shape[0], blocks[0][1].device
            R = torch.eye(N, dtype=dtype, device=dev).expand(B, N, N).contiguous()
        Abar = torch.zeros((B, N, N), dtype=dtype, device=dev)
        for c0, A in blocks:
            Abar[:, c0:c0 + A.shape[1], c0:c0 + A.shape[1]] = A.to(dtype)
        R = alpha * R + beta * (Abar @ R)
    return R[:, q0:q0 + nq].contiguous()


def relevance_heatmaps(R, T, grid):
    """Relevance rows R [B, nq, T + 1 + grid^2] of an image-text pass (text first, then the image CLS, then the patches row
    by row; T = 0 for an image-only pass) -> (text [B, nq, T], image [B, nq, grid, grid]).  The image-CLS column T is left
    out, as in text_to_image_heatmaps.  Nothing is normalised: display code min-max normalises."""
    if R.dim() != 3 or T < 0 or grid < 1 or R.shape[2] != T + 1 + grid * grid:
        raise ValueError(f'need relevance rows [B, nq, {T + 1 + grid * grid}] (T={T}, grid={grid}), got {tuple(R.shape)}')
    return R[:, :, :T], R[:, :, T + 1:].reshape(R.shape[0], R.shape[1], grid, grid)


def relevance_capture(block, state, T, alpha, beta):
    """The engine.BlockMeta.capture callback of one block call for method 'gradcam': the head-mean 'cam' map of the block
    (every query row) from the engine's buffers, multiplied into the rows state['X'] at once -- the backward reaches the
    captured layers top-down, which is the order the row form needs, so one Abar is alive at a time."""
    def capture(qkv, dctx, plan, fused):
        kinds = plan_kinds(plan, fused)
        maps = {name: attention_gradcam(qkv, dctx, seg, plan.B, n, block.num_heads, plan.keymask, block.attn.scale,
                                        None, True, 'cam') for name, seg, n in kinds}
        state['X'] = relevance_propagate(state['X'], maps[None] if len(kinds) == 1 else maps, T, alpha, beta)
    return capture
