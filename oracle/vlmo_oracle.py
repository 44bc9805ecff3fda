"""Plain-PyTorch fp32 restatement of the VLMO backbone (TEST INFRASTRUCTURE).

Functional: every function takes the backbone state dict ``sd`` (keys as in
the reference) so that autograd on ``sd`` tensors with
``requires_grad`` gives reference gradients.  Eval-mode semantics (dropout and
drop-path are identities), i.e. the configuration the parity tests pin, unless a
caller hands in the randomness of a training pass explicitly (``Train`` below).

Follows, line by line:
  * LayerNorm eps=1e-12           models/vlmo/vlmo_module.py:21-23, vlmo.py:26-36
  * Attention.forward             models/vlmo/vlmo.py:68-98
  * Block.forward                 models/vlmo/vlmo.py:187-197
  * timm Mlp (fc1, GELU-erf, fc2) models/vlmo/vlmo.py:141-157 (third party)
  * VLMO.embed_img / embed_txt    models/vlmo/vlmo.py:298-324
  * transformers BertEmbeddings   word + type[0] + pos[0:T] -> LN(1e-12)
  * VLMO.forward_features         models/vlmo/vlmo.py:357-414
  * VLMO.forward_interval         models/vlmo/vlmo.py:326-355
  * BertPooler                    tanh(W x[:,0] + b), vlmo_module.py:379
"""
import contextlib

import torch
import torch.nn.functional as F

LN_EPS = 1e-12

# ---- bf16-operand mode (round 4): the same restatement with every matrix-product OPERAND rounded to bf16 at the points
# where the HIP engine holds bf16 (LayerNorm outputs, qkv, soft-max probabilities, attention context, GELU output, weight
# shadows, image patches) and fp32 everywhere else (accumulation, bias, residual stream, LayerNorm / soft-max statistics,
# GELU argument).  What is left between the engine and THIS oracle is summation order and the rare value that sits on a
# rounding boundary, so the comparison can be held to ~1e-3 instead of the ~3e-2 that bf16 operands cost against the fp32
# restatement: a wrong tile or a missed term no longer hides under rounding noise.  Activation gradients are rounded at
# the same points on the way back (the engine's dy1 / dqkv / dctx / du are bf16 GEMM operands too); parameter gradients
# stay fp32.  The fp32 mode above remains the restatement that is pinned to the reference.
_BF16 = [False]


@contextlib.contextmanager
def bf16_operands(enabled=True):
    prev = _BF16[0]
    _BF16[0] = bool(enabled)
    try:
        yield
    finally:
        _BF16[0] = prev


class _RoundAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().float()

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().float()


class _RoundWeight(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w):
        return w.bfloat16().float()

    @staticmethod
    def backward(ctx, g):
        return g


def _ra(x):
    return _RoundAct.apply(x) if _BF16[0] else x


def _rw(w):
    return _RoundWeight.apply(w) if _BF16[0] else w


def layer_norm(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, LN_EPS)


class Train:
    """The randomness of ONE training-mode Block call, handed in instead of drawn (no generator is touched, so no
    caller has to mirror an order of draws).  Keep masks are bool, True = kept; a kept element is multiplied by
    ``inv_keep`` = 1 / (1 - p) (nn.Dropout), a dropped one is zero:
      attn  [B, heads, N, N]  attention probabilities after the soft-max        vlmo.py:93
      proj  [B, N, d]         output of the attention projection                vlmo.py:97
      gelu  [B, N, hidden]    timm Mlp: after the activation
      fc2   [B, N, d]         timm Mlp: after fc2
    scale1 / scale2 [B]: timm DropPath of the attention / FFN residual branch, one factor per sample (0 or 1 / keep;
    vlmo.py:132-133, 194-196), None = no drop-path.  attn_inv_keep defaults to inv_keep (attn_drop_rate == drop_rate).
    Any mask may be None (that site is the identity)."""

    def __init__(self, attn=None, proj=None, gelu=None, fc2=None, inv_keep=1.0, scale1=None, scale2=None,
                 attn_inv_keep=None):
        self.attn, self.proj, self.gelu, self.fc2 = attn, proj, gelu, fc2
        self.inv_keep = float(inv_keep)
        self.attn_inv_keep = float(inv_keep if attn_inv_keep is None else attn_inv_keep)
        self.scale1, self.scale2 = scale1, scale2

    def replace(self, **kw):
        new = Train.__new__(Train)
        new.__dict__.update(self.__dict__)
        new.__dict__.update(kw)
        return new


def _dropout(x, keep, inv_keep):
    """nn.Dropout with the mask given: keep None = identity"""
    return x if keep is None else x * (keep.to(x.dtype) * inv_keep)


def _drop_path(x, scale):
    """timm DropPath with the per-sample factor given ([B], broadcast over the sample's tokens)"""
    return x if scale is None else x * scale.to(x.dtype).view(-1, *([1] * (x.dim() - 1)))


def attention(sd, p, x, mask, num_heads, train=None):
    """vlmo.py:68-98.  Returns (out, attn_probs); with ``train`` (a Train) the probabilities are the post-dropout
    ones, as the reference returns them in training mode."""
    B, N, C = x.shape
    dh = C // num_heads
    qkv_bias = None             # qkv_bias=False: no q_bias / v_bias parameters (vlmo.py:57-62, 70-75)
    if p + 'q_bias' in sd:
        qkv_bias = torch.cat((sd[p + 'q_bias'],
                              torch.zeros_like(sd[p + 'v_bias']),
                              sd[p + 'v_bias']))
    qkv = _ra(F.linear(x, _rw(sd[p + 'qkv.weight']), qkv_bias))
    qkv = qkv.reshape(B, N, 3, num_heads, dh).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    attn = (q @ k.transpose(-2, -1)) * dh ** -0.5
    if mask is not None:
        attn = attn.masked_fill(~mask.bool()[:, None, None, :], float('-inf'))
    attn = attn.softmax(dim=-1)
    if train is not None:
        attn = _dropout(attn, train.attn, train.attn_inv_keep)
    x = _ra((_ra(attn) @ v).transpose(1, 2).reshape(B, N, C))
    x = F.linear(x, _rw(sd[p + 'proj.weight']), sd[p + 'proj.bias'])
    if train is not None:
        x = _dropout(x, train.proj, train.inv_keep)
    return x, attn


def mlp(sd, p, x, train=None):
    """timm Mlp: fc1, GELU, drop, fc2, drop (the two drops are identities without ``train``)."""
    h = F.gelu(F.linear(x, _rw(sd[p + 'fc1.weight']), sd[p + 'fc1.bias']))
    if train is not None:
        h = _dropout(h, train.gelu, train.inv_keep)
    y = F.linear(_ra(h), _rw(sd[p + 'fc2.weight']), sd[p + 'fc2.bias'])
    if train is not None:
        y = _dropout(y, train.fc2, train.inv_keep)
    return y


def block(sd, i, x, mask, route, num_heads, train=None):
    """vlmo.py:187-197 (both branches).  Without ``train``: eval mode, DropPath = identity; with it (a Train): the
    four dropouts and the two DropPath factors of a training-mode call."""
    p = f'blocks.{i}.'
    a, _ = attention(sd, p + 'attn.',
                     _ra(layer_norm(x, sd[p + 'norm1.weight'], sd[p + 'norm1.bias'])),
                     mask, num_heads, train)
    has_gamma = p + 'gamma_1' in sd         # init_values=None: no layer-scale (vlmo.py:158-162, 190-192)
    a = sd[p + 'gamma_1'] * a if has_gamma else a
    x = x + (a if train is None else _drop_path(a, train.scale1))
    m = mlp(sd, p + f'mlp.{route}.',
            _ra(layer_norm(x, sd[p + 'norm2.weight'], sd[p + 'norm2.bias'])), train)
    m = sd[p + 'gamma_2'] * m if has_gamma else m
    x = x + (m if train is None else _drop_path(m, train.scale2))
    return x


def embed_img(sd, mc, img, bool_masked_pos=None, img_token_type_idx=1, keep=None, inv_keep=1.0):
    """vlmo.py:298-319 with timm PatchEmbed = conv(k=s=patch).flatten(2).T.  keep (bool [B, P, d], optional): the
    mask of pos_drop (vlmo.py:316), applied after the position embedding and before the token type is added."""
    x = F.conv2d(_ra(img), _rw(sd['patch_embed.proj.weight']), sd['patch_embed.proj.bias'],
                 stride=mc.patch_size)
    x = x.flatten(2).transpose(1, 2)
    B, S, _ = x.shape
    if bool_masked_pos is not None:
        w = bool_masked_pos.reshape(B, -1).unsqueeze(-1).type_as(x)
        x = x * (1 - w) + sd['img_mask_token'].expand(B, S, -1) * w
    x = torch.cat((sd['img_cls_token'].expand(B, -1, -1), x), dim=1)
    x = x + sd['pos_embed']
    if keep is not None:
        x = _dropout(x, keep, inv_keep)
    x = x + sd['token_type_embeddings.weight'][img_token_type_idx]
    return x


def embed_txt(sd, mc, ids, keep=None, inv_keep=1.0):
    """vlmo.py:321-324; BertEmbeddings with token_type_ids = 0, positions 0..T-1.  keep (bool [B, T, d], optional):
    the mask of BertEmbeddings' dropout, applied to the LayerNorm output before the token type is added."""
    T = ids.shape[1]
    # BertEmbeddings.word_embeddings has padding_idx=0: row 0 is looked up like any
    # other row in forward but receives no gradient.
    e = F.embedding(ids, sd['txt_embeddings.word_embeddings.weight'], padding_idx=0)
    e = e + sd['txt_embeddings.token_type_embeddings.weight'][0]
    e = e + sd['txt_embeddings.position_embeddings.weight'][:T]
    e = layer_norm(e, sd['txt_embeddings.LayerNorm.weight'],
                   sd['txt_embeddings.LayerNorm.bias'])
    if keep is not None:
        e = _dropout(e, keep, inv_keep)
    return e + sd['token_type_embeddings.weight'][0]


def forward_features(sd, mc, img=None, txt=None, img_attn_masks=None,
                     txt_attn_masks=None, bool_masked_pos=None,
                     fusion_layer=None, img_token_type_idx=1,
                     return_intermediates=False):
    """vlmo.py:357-414.  Returns (x, mask) (+ per-block outputs if asked)."""
    h, L = mc.num_heads, mc.depth
    inter = []
    final = lambda x: layer_norm(x, sd['norm.weight'], sd['norm.bias'])
    if txt is None:
        x = embed_img(sd, mc, img, bool_masked_pos, img_token_type_idx)
        for i in range(L):
            x = block(sd, i, x, img_attn_masks, 'v', h)
            inter.append(x)
        out = (final(x), img_attn_masks)
        return out + (inter,) if return_intermediates else out
    if img is None:
        x = embed_txt(sd, mc, txt)
        for i in range(L):
            x = block(sd, i, x, txt_attn_masks, 'l', h)
            inter.append(x)
        out = (final(x), txt_attn_masks)
        return out + (inter,) if return_intermediates else out
    xi = embed_img(sd, mc, img, bool_masked_pos, img_token_type_idx)
    xt = embed_txt(sd, mc, txt)
    Fl = fusion_layer or mc.fusion_layer
    assert 0 <= Fl <= L
    for i in range(Fl):
        xi = block(sd, i, xi, img_attn_masks, 'v', h)
        xt = block(sd, i, xt, txt_attn_masks, 'l', h)
        inter.append(torch.cat([xt, xi], dim=1))
    x = torch.cat([xt, xi], dim=1)          # text first: vlmo.py:406
    m = torch.cat([txt_attn_masks, img_attn_masks], dim=1)
    for i in range(Fl, L):
        x = block(sd, i, x, m, 'vl', h)
        inter.append(x)
    out = (final(x), m)
    return out + (inter,) if return_intermediates else out


def forward_interval(sd, mc, x, attn_masks, route, need_embed=False,
                     bool_masked_pos=None, in_layer=None, out_layer=None,
                     img_token_type_idx=1, need_norm=False):
    """vlmo.py:326-355."""
    assert route in ['v', 'l', 'vl']
    if need_embed:
        if route == 'v':
            if attn_masks is None:
                attn_masks = torch.ones(x.shape[0], (mc.img_size // mc.patch_size) ** 2 + 1,
                                        dtype=torch.int64)
            x = embed_img(sd, mc, x, bool_masked_pos, img_token_type_idx)
        elif route == 'l':
            x = embed_txt(sd, mc, x)
    for i in list(range(mc.depth))[in_layer:out_layer]:
        x = block(sd, i, x, attn_masks, route, mc.num_heads)
    return layer_norm(x, sd['norm.weight'], sd['norm.bias']) if need_norm else x


def pooler(sd, x):
    return torch.tanh(F.linear(x[:, 0], sd['pooler.dense.weight'],
                               sd['pooler.dense.bias']))
