"""Image-text retrieval evaluation on the ITC features of the dual encoder (the Flickr30K / COCO recall@K VLMo reports;
upstream names the task in conf/train/finetune_retrieval.yaml and leaves compute_irtr_recall empty).

Training for it is the existing ITC objective (``loss_names = ['itc']``, optionally ``global_reduce``).  This module is
the evaluation: encode a gallery, rank it, count recall.  The ranking of CUDA tensors is hip.sim_topk (fp32 MFMA similarity
fused with the top-K selection: the [N_query, N_gallery] score matrix never exists); CPU tensors take a torch restatement
with the same ordering rule, which is what the tests compare the kernel with.  Single process only.
"""
import torch

from . import hip

# the CPU restatement never holds more than this many scores (fp64) at once
_CPU_SLAB = 1 << 22


def _itc_head(model):
    head = getattr(model, 'itc_head', None)
    if head is None:
        raise ValueError("retrieval needs the ITC head: build the model with 'itc' in train.loss_names")
    return head


def _encode(model, n, chunk_batch, infer_mode, route, batch_size, ragged=False):
    head = _itc_head(model)
    if batch_size < 1:
        raise ValueError('batch_size must be >= 1')
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            feats = []
            for b0 in range(0, n, batch_size):
                co = model.infer(chunk_batch(b0, min(n, b0 + batch_size)), infer_mode=infer_mode,
                                 ragged=ragged)['co_feats']
                f = head(co[:, 0], route)               # unit rows (heads.ITCHead)
                if f.dtype != torch.float32:            # half-precision head under autocast: unit length in fp32
                    f = torch.nn.functional.normalize(f.float(), dim=-1)
                feats.append(f)
            return torch.cat(feats, 0)
    finally:
        model.train(was_training)


def encode_images(model, images, batch_size=64):
    """images [N, C, H, W] -> L2-normalised fp32 ITC features [N, itc_dim] (eval mode, no gradients)."""
    return _encode(model, images.shape[0], lambda a, b: {'image': images[a:b]}, 'img_only', 'v', batch_size)


def encode_texts(model, text_ids, text_mask, batch_size=256, ragged=False):
    """text_ids, text_mask [N, T] -> L2-normalised fp32 ITC features [N, itc_dim] (eval mode, no gradients).

    ragged=True runs every text with the positions up to its last unmasked one only (VLMO.forward_features' txt_lens):
    the [CLS] feature is the padded pass's up to the summation order inside attention.  The lengths come from the host
    when text_mask is a CPU tensor (it is then uploaded chunk by chunk); a mask that lives on the device is read back ONCE per call (a device-to-host
    synchronisation: this is an evaluation utility, not a training step)."""
    lens = None
    if ragged:
        from .objectives import attach_text_lens
        lens = attach_text_lens({'text_mask': text_mask.cpu()})['_txt_lens']

    def chunk(a, b):
        out = {'text_ids': text_ids[a:b], 'text_mask': text_mask[a:b].to(text_ids.device)}     # a host mask is uploaded
        if lens is not None:
            out['_txt_lens'] = lens[a:b]
        return out

    return _encode(model, text_ids.shape[0], chunk, 'txt_only', 'l', batch_size, ragged=ragged)


def _sim_topk_cpu(q, g, k, scale, chunk_rows=None):
    """The ordering rule of vlmo_sim_topk restated in torch: scores in fp64 rounded to fp32, higher first, equal scores by
    ascending gallery index (a stable sort keeps them in index order), -inf / -1 past the gallery's end.  Queries go in
    slabs of at most _CPU_SLAB scores (``chunk_rows`` overrides the slab height)."""
    Nq, Ng = q.shape[0], g.shape[0]
    rows = chunk_rows if chunk_rows else max(1, _CPU_SLAB // max(1, Ng))
    kk = min(k, Ng)
    val = torch.full((Nq, k), float('-inf'), dtype=torch.float32)
    idx = torch.full((Nq, k), -1, dtype=torch.int64)
    gd = g.double().t()
    for r0 in range(0, Nq, rows):
        s = ((q[r0:r0 + rows].double() @ gd) * scale).float()
        sv, si = torch.sort(s, dim=1, descending=True, stable=True)
        val[r0:r0 + rows, :kk] = sv[:, :kk]
        idx[r0:r0 + rows, :kk] = si[:, :kk]
    return val, idx


def sim_topk(q, g, k, scale=1.0, splits=0):
    """The k best rows of g [Ng, D] for every row of q [Nq, D] under score = scale * <q, g> -> (values fp32 [Nq, k],
    indices int64 [Nq, k]), best first; among equal scores the lower gallery index first; with Ng < k the tail is
    -inf / -1.  Limits (include/vlmo_hip.h: vlmo_sim_topk): 1 <= k <= 16, 4 <= D <= 1024, D % 4 == 0, scale > 0, fp32.
    ``splits``: gallery slices of the HIP kernel (0 = chosen by the library); the result does not depend on it."""
    if q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
        raise ValueError('sim_topk: q [Nq, D] and g [Ng, D] must be 2-D with the same width')
    if q.dtype != torch.float32 or g.dtype != torch.float32:
        raise ValueError('sim_topk: fp32 features only (bf16 cannot resolve the score gaps recall@1 is decided by)')
    if q.device != g.device:
        raise ValueError('sim_topk: q and g must be on the same device')
    D = q.shape[1]
    if not (1 <= k <= 16 and 4 <= D <= 1024 and D % 4 == 0 and scale > 0 and q.shape[0] >= 1 and g.shape[0] >= 1):
        raise ValueError(f'sim_topk: need 1 <= k <= 16, 4 <= D <= 1024, D % 4 == 0, scale > 0 and non-empty q, g '
                         f'(k={k}, D={D}, scale={scale}, Nq={q.shape[0]}, Ng={g.shape[0]})')
    if q.is_cuda:
        if q.stride(1) != 1:
            q = q.contiguous()
        if g.stride(1) != 1:
            g = g.contiguous()
        val, idx = hip.sim_topk(q, g, k, scale, splits)
        return val, idx.long()
    return _sim_topk_cpu(q, g, k, scale)


def recall_at_k(indices, txt2img, direction, ks=(1, 5, 10)):
    """Recall@k of ranked lists -> fp32 tensor [len(ks)] of fractions in [0, 1] on the inputs' device.
    indices int64 [N_query, K] from sim_topk (-1 = no entry); txt2img int64 [N_txt]: the image of every caption.
    't2i': queries are captions, entries are images; query t hits at k if txt2img[t] is among its first k entries.
    'i2t': queries are images, entries are captions; query i hits at k if a caption c among its first k entries has
    txt2img[c] == i (an image without a caption never hits)."""
    if direction not in ('t2i', 'i2t'):
        raise ValueError("direction must be 't2i' or 'i2t'")
    if max(ks) > indices.shape[1]:
        raise ValueError(f'recall@{max(ks)} needs {max(ks)} ranked entries per query, got {indices.shape[1]}')
    txt2img = txt2img.to(indices.device)
    if direction == 't2i':
        if indices.shape[0] != txt2img.shape[0]:
            raise ValueError('t2i: one ranked list per caption expected')
        match = indices == txt2img[:, None]
    else:
        owner = txt2img[indices.clamp(min=0)]
        match = (owner == torch.arange(indices.shape[0], device=indices.device)[:, None]) & (indices >= 0)
    first = match.float().cumsum(1) > 0                 # column j: a hit within the first j + 1 entries
    cols = torch.tensor([k - 1 for k in ks], device=indices.device)
    return first[:, cols].float().mean(0)


def evaluate_retrieval(model, images, text_ids, text_mask, txt2img, ks=(1, 5, 10), image_batch_size=64,
                       text_batch_size=256, scale=1.0, splits=0, ragged_text=False):
    """Recall of both directions for a gallery of images and captions -> {'ir_r<k>': text-to-image, 'tr_r<k>':
    image-to-text for k in ks, 'r_mean': their mean} (ViLT's / VLMo's metric names) as Python floats.  Two sim_topk calls,
    one device-to-host read.  ragged_text: encode_texts' ``ragged`` (one more read when text_mask lives on the device)."""
    i_feat = encode_images(model, images, image_batch_size)
    t_feat = encode_texts(model, text_ids, text_mask, text_batch_size, ragged=ragged_text)
    return recall_from_features(i_feat, t_feat, txt2img, ks, scale, splits)


def recall_from_features(i_feat, t_feat, txt2img, ks=(1, 5, 10), scale=1.0, splits=0):
    """evaluate_retrieval from encoded features: i_feat [N_img, D], t_feat [N_txt, D] fp32 on one device."""
    kmax = max(ks)
    _, t2i = sim_topk(t_feat, i_feat, kmax, scale, splits)
    _, i2t = sim_topk(i_feat, t_feat, kmax, scale, splits)
    ir = recall_at_k(t2i, txt2img, 't2i', ks)
    tr = recall_at_k(i2t, txt2img, 'i2t', ks)
    both = torch.cat([ir, tr])
    flat = torch.cat([both, both.mean()[None]]).tolist()
    out = {f'ir_r{k}': flat[j] for j, k in enumerate(ks)}
    out.update({f'tr_r{k}': flat[len(ks) + j] for j, k in enumerate(ks)})
    out['r_mean'] = flat[-1]
    return out
