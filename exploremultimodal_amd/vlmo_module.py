"""Host-side mirror of VlmoModule (models/vlmo/vlmo_module.py:14-442): same constructor
(attribute-style config), parameter names, `infer` / `forward` / `load_from_ckpt` /
`no_weight_decay` contracts.  Pretraining losses [mlm, mim, itc, itm] and the VQAv2 fine-tuning
loss [vqa] (the classifier and its loss on the HIP path of heads.VQAHeadFn).  With train.isda_lambda > 0
the classifier's last Linear becomes ``vqa_last`` and ``isda_head`` keeps the ISDA estimator (buffers
isda_head.estimator.{count, mean, cov}); training steps with answers run heads.VQAIsdaHeadFn.  ISDA
needs train.epochs and train.cur_epoch (its ratio) and is refused with R-Drop (kl_alpha > 0), which
fails upstream.  Each rank keeps its own estimator, as the reference's DDP with broadcast_buffers=False
does.  The other downstream heads (nlvr2 / irtr / mpp / refcoco), the momentum twin (vlmo_ema; the plain
weight average model_ema is ema.ModelEma) and the negative queue raise
NotImplementedError (out of scope, off in conf/train/pretrain_mum.yaml and
conf/train/finetune_vqa.yaml)."""
import math
from collections import defaultdict
from functools import partial

import numpy as np

import torch
import torch.nn as nn

from . import attnmap, objectives
from .heads import ISDAHead, ITCHead, ITMHead, MIMHead, MLMHead
from .vlmo import VLMO, LayerNorm


class VlmoModule(nn.Module):

    def __init__(self, config):
        super().__init__()
        self.config = config
        model_cfg = config.model
        norm_layer = partial(LayerNorm, eps=1e-12, export='fused' not in model_cfg.norm_layer)
        self.transformer = VLMO(
            img_size=model_cfg.img_size, patch_size=model_cfg.patch_size, in_chans=model_cfg.in_chans,
            num_classes=model_cfg.num_classes, embed_dim=model_cfg.embed_dim, depth=model_cfg.depth,
            num_heads=model_cfg.num_heads, mlp_ratio=model_cfg.mlp_ratio, qkv_bias=model_cfg.qkv_bias,
            qk_scale=None, drop_rate=model_cfg.drop_rate, attn_drop_rate=model_cfg.attn_drop_rate,
            drop_path_rate=model_cfg.drop_path_rate, norm_layer=norm_layer, init_values=model_cfg.init_values,
            vocab_size=model_cfg.vocab_size, max_text_len=model_cfg.max_text_len,
            fusion_layer=model_cfg.fusion_layer)
        self._freeze_params()

        self.loss_names = config.train.loss_names
        hs = model_cfg.embed_dim
        for unsupported in ('mpp', 'nlvr2', 'irtr', 'refcoco'):
            if unsupported in self.loss_names:
                raise NotImplementedError(f'loss {unsupported!r} belongs to a downstream phase this engine does not '
                                          'implement (pretraining and VQAv2 fine-tuning only)')
        if 'mlm' in self.loss_names:
            self.mlm_head = MLMHead(self.transformer.bert_config,
                                    weight=self.transformer.txt_embeddings.word_embeddings.weight)
            self.mlm_head.apply(self.transformer._init_weights)
        if 'itc' in self.loss_names:
            self.itc_head = ITCHead(hs, model_cfg.itc_dim)
            self.itc_head.apply(self.transformer._init_weights)
            self.itc_temp = nn.Parameter(torch.ones([]) * np.log(1 / model_cfg.itc_temp))
        if 'itm' in self.loss_names:
            self.itm_head = ITMHead(hs)
            self.itm_head.apply(self.transformer._init_weights)
        if 'mim' in self.loss_names:
            self.d_vae = objectives.create_d_vae(weight_path=config.train.discrete_vae_weight_path,
                                                 d_vae_type=config.train.discrete_vae_type, device='cpu',
                                                 image_size=model_cfg.img_size // 2,
                                                 vocab_size=model_cfg.img_vocab_size)
            for p in self.d_vae.parameters():
                p.requires_grad = False
            self.mim_head = MIMHead(hs, model_cfg.img_vocab_size)
            self.mim_head.apply(self.transformer._init_weights)
        if 'vqa' in self.loss_names:                     # vlmo_module.py:85-101
            isda_lambda = getattr(config.train, 'isda_lambda', 0.0)
            if isda_lambda > 0.:
                missing = [f for f in ('epochs', 'cur_epoch') if not hasattr(config.train, f)]
                if missing:
                    raise NotImplementedError(
                        f'isda_lambda > 0 needs train.epochs and train.cur_epoch: the ISDA ratio is isda_lambda * '
                        f'cur_epoch / epochs (objectives.py:327-335); this config lacks {", ".join(missing)}')
                if getattr(config.train, 'kl_alpha', 0.0) > 0.:
                    raise NotImplementedError(
                        'isda_lambda > 0 with kl_alpha > 0 (R-Drop) is not supported: upstream the second pass feeds '
                        'the 3-layer classifier output to the BCE loss, which fails on its shape')
            vs = config.data.vqav2_label_size
            self.vqa_classifier = nn.Sequential(nn.Linear(hs, hs * 2), norm_layer(hs * 2), nn.GELU(), nn.Linear(hs * 2, vs))
            self.vqa_classifier.apply(self.transformer._init_weights)
            self.vqa_last = None
            if isda_lambda > 0.:
                self.vqa_last = self.vqa_classifier[-1]
                self.vqa_classifier = self.vqa_classifier[:-1]
                self.isda_head = ISDAHead(hidden_size=hs * 2, class_num=vs)

        self.transformer_m = None
        if getattr(self.config, 'vlmo_ema', False):
            raise NotImplementedError('vlmo_ema (the momentum twin transformer_m / itc_head_m and the momentum ITC '
                                      'branch) is out of scope; config.yaml:136 default is off.  The plain weight '
                                      'average (model_ema) is exploremultimodal_amd.ema.ModelEma')
        if hasattr(config.train, 'neg_queue') and config.train.neg_queue:
            raise NotImplementedError('neg_queue is out of scope; pretrain_mum.yaml:40 default is off')
        self.q_size = 0
        self.img_queue, self.txt_queue = None, None

    def _freeze_params(self):
        """vlmo_module.py:148-167."""
        if self.config.train.phase in ['pretrain_txt']:
            for b in self.transformer.blocks:
                del b.mlp['vl']
                if self.config.train.fixed_attn:
                    b.gamma_1.requires_grad = False
                    b.gamma_2.requires_grad = False
                    for p in b.attn.parameters():
                        p.requires_grad = False
                    for p in b.norm1.parameters():
                        p.requires_grad = False
                    for p in b.norm2.parameters():
                        p.requires_grad = False
            for p in self.transformer.norm.parameters():
                p.requires_grad = False
        elif self.config.train.phase in ['pretrain_mum', 'finetune_vqa']:
            for b in self.transformer.blocks[:self.transformer.fusion_layer]:
                del b.mlp['vl']

    def _adjust_downstream_params(self):
        """vlmo_module.py:169-185: only touches nlvr2 / irtr heads, which this module never builds."""

    # ------------------------------------------------------------- checkpoints
    def interpolate_pos_embedding(self, state_dict):
        """Fit a checkpoint's position tables to this model (behaviour of vlmo_module.py:187-232): the image table is
        resampled bicubically when the checkpoint was trained on another patch grid (class / extra tokens kept as they
        are), the text table is cut to ``max_text_len`` rows."""
        tr = self.transformer
        grid = math.isqrt(tr.patch_embed.num_patches)
        n_extra = tr.pos_embed.shape[-2] - tr.patch_embed.num_patches
        for key in ('pos_embed', 'transformer.pos_embed'):
            table = state_dict.get(key)
            if table is None:
                continue
            src = math.isqrt(table.shape[-2] - n_extra)
            if src == grid:
                continue
            head, body = table[:, :n_extra], table[:, n_extra:]
            body = body.unflatten(1, (src, src)).movedim(-1, 1)                       # [1, C, src, src]
            body = torch.nn.functional.interpolate(body, size=(grid, grid), mode='bicubic', align_corners=False)
            state_dict[key] = torch.cat([head, body.movedim(1, -1).flatten(1, 2)], dim=1)
        txt = 'transformer.txt_embeddings.position_embeddings.weight'
        if txt in state_dict:
            state_dict[txt] = state_dict[txt][:tr.max_text_len]
        state_dict.pop('transformer.txt_embeddings.position_ids', None)   # non-persistent buffer upstream
        return state_dict

    def _load_vlmo(self, state_dict):
        for k in list(state_dict.keys()):
            for old, new in (('.mlp.v_mlp', '.mlp.v'), ('.mlp.l_mlp', '.mlp.l'), ('.mlp.vl_mlp', '.mlp.vl')):
                if old in k:
                    state_dict[k.replace(old, new)] = state_dict.pop(k)
                    break
        matching = self.load_state_dict(state_dict, strict=False)
        self._adjust_downstream_params()
        return matching

    def _load_beit(self, state_dict):
        for k in list(state_dict.keys()):
            nk = k
            if 'mlp' in nk:
                nk = nk.replace('.mlp', '.mlp.v')
            if 'mask_token' in nk:
                nk = nk.replace('mask_token', 'img_mask_token')
            elif 'cls_token' in nk:
                nk = nk.replace('cls_token', 'img_cls_token')
            if 'lm_head' in nk:
                nk = nk.replace('lm_head', 'fc')
            if nk != k:
                state_dict[nk] = state_dict.pop(k)
        if 'mim' in self.loss_names:
            self.mim_head.load_state_dict(state_dict, strict=False)
        matching = self.transformer.load_state_dict(state_dict, strict=False)
        self._adjust_downstream_params()
        return matching

    def load_from_ckpt(self, state_dict):
        """vlmo_module.py:300-319 -> (matching, is_beit)."""
        state_dict = self.interpolate_pos_embedding(state_dict)
        is_beit = not any(('.mlp.v' in k or '.mlp.l' in k or '.mlp.vl' in k) for k in state_dict)
        matching = (self._load_beit if is_beit else self._load_vlmo)(state_dict)
        return matching, is_beit

    # ------------------------------------------------------------------ infer
    def _text_lens(self, batch, ragged=None):
        """(txt_lens, txt_off) for a pass over the batch's texts, or (None, None) = every text at full width.
        ``config.train.ragged_text`` (not a reference option, default off) or ``ragged=True`` turns variable-length text
        on; the lengths are those objectives.attach_text_lens put on the HOST batch (``_txt_lens``, a tuple of python
        ints), so no pass asks the device.  A batch without them runs padded."""
        if ragged is None:
            ragged = bool(getattr(self.config.train, 'ragged_text', False))
        lens = batch.get('_txt_lens') if ragged else None
        if lens is None:
            return None, None
        off, ids = batch.get('_txt_off'), batch.get('text_ids')
        if not (torch.is_tensor(off) and torch.is_tensor(ids) and off.device == ids.device):
            off = None
        return lens, off

    def infer(self, batch, infer_mode='img-txt', mask_txt=False, mask_img=False, image_token_type_idx=1,
              momentum_mode=False, ragged=None):
        """vlmo_module.py:321-393.  ``ragged``: see _text_lens (None = config.train.ragged_text)."""
        assert infer_mode in ['img_only', 'txt_only', 'img-txt']
        if momentum_mode:
            assert self.transformer_m is not None
        transformer = self.transformer
        img, img_attn_masks, bool_masked_pos = None, None, None
        txt_ids, txt_labels, txt_attn_masks = None, None, None
        txt_lens, txt_off = None, None
        if 'img' in infer_mode:
            imgkey = f'image_{image_token_type_idx - 1}' if f'image_{image_token_type_idx - 1}' in batch else 'image'
            img = batch[imgkey]
            B = img.size(0)
            img_attn_masks = torch.ones([B, transformer.patch_embed.num_patches + 1], dtype=torch.int64,
                                        device=img.device)
            bool_masked_pos = batch['image_bool_masked_pos'] if mask_img else None
        if 'txt' in infer_mode:
            do_mlm = '_mlm' if mask_txt else ''
            txt_ids = batch[f'text_ids{do_mlm}']
            txt_labels = batch[f'text_labels{do_mlm}'] if mask_txt else None
            txt_attn_masks = batch['text_mask']
            txt_lens, txt_off = self._text_lens(batch, ragged)
        co_feats, _ = transformer.forward_features(img=img, txt=txt_ids, img_attn_masks=img_attn_masks,
                                                   txt_attn_masks=txt_attn_masks, bool_masked_pos=bool_masked_pos,
                                                   fusion_layer=None, txt_lens=txt_lens, txt_off=txt_off)
        if txt_ids is not None:
            txt_feats, img_feats = (co_feats[:, :transformer.max_text_len], co_feats[:, transformer.max_text_len:])
        else:
            txt_feats, img_feats = None, co_feats
        cls_feats = transformer.pooler(co_feats)
        return {'txt_feats': txt_feats, 'img_feats': img_feats, 'co_feats': co_feats, 'cls_feats': cls_feats,
                'img_masks': img_attn_masks, 'img_bool_masked_pos': bool_masked_pos, 'txt_labels': txt_labels,
                'txt_ids': txt_ids, 'txt_masks': txt_attn_masks}

    def attention_maps(self, batch, infer_mode='img-txt', layers=None, queries=None, head_mean=False):
        """The attention maps of the backbone pass ``infer(batch, infer_mode)`` runs -> {layer: map} (VLMO.attention_maps:
        shapes, zero rules, eval mode only).  Masks and inputs are picked exactly as infer picks them."""
        assert infer_mode in ['img_only', 'txt_only', 'img-txt']
        transformer = self.transformer
        img, img_attn_masks, txt_ids, txt_attn_masks = None, None, None, None
        if 'img' in infer_mode:
            img = batch['image_0'] if 'image_0' in batch else batch['image']
            img_attn_masks = torch.ones([img.size(0), transformer.patch_embed.num_patches + 1], dtype=torch.int64,
                                        device=img.device)
        if 'txt' in infer_mode:
            txt_ids, txt_attn_masks = batch['text_ids'], batch['text_mask']
        return transformer.attention_maps(img=img, txt=txt_ids, img_attn_masks=img_attn_masks,
                                          txt_attn_masks=txt_attn_masks, layers=layers, queries=queries,
                                          head_mean=head_mean)

    def attention_gradcam(self, batch, infer_mode='img-txt', layers=None, target='itm', queries=None, head_mean=False,
                          kind='cam'):
        """Gradient-weighted attention maps of the backbone pass ``infer(batch, infer_mode)`` runs -> {layer: map}
        (VLMO.attention_gradcam: kinds, shapes, eval mode only).  target='itm': the score is the "match" logit
        itm_head(cls_feats)[:, 1], summed over the batch -- in eval mode nothing couples the samples, so every sample
        gets the gradient of its own logit; needs 'itm' among the losses.  A callable target gets the dict infer returns
        and gives a scalar tensor.  Masks and inputs are picked exactly as infer picks them."""
        kw, score_fn = self._gradcam_inputs('attention_gradcam', batch, infer_mode, target)
        return self.transformer.attention_gradcam(score_fn, layers=layers, queries=queries, head_mean=head_mean, kind=kind,
                                                  **kw)

    def _gradcam_inputs(self, what, batch, infer_mode, target, need_score=True):
        """What attention_gradcam and attention_relevance share: the inputs and masks infer picks, as keyword arguments
        of the transformer's entry point, and the score function of ``target`` (need_score=False: target is not looked
        at and the score function is None)."""
        assert infer_mode in ['img_only', 'txt_only', 'img-txt']
        if self.training:
            raise RuntimeError(f'{what} needs eval mode: the maps are pre-dropout and are computed from the '
                               'activations of a deterministic pass (call model.eval() first)')
        if need_score and target == 'itm':
            if 'itm' not in self.loss_names:
                raise ValueError("target='itm' needs the ITM head: build the model with 'itm' in train.loss_names")
        elif need_score and not callable(target):
            raise ValueError(f"target must be 'itm' or a callable on the dict infer returns, got {target!r}")
        transformer = self.transformer
        img, img_attn_masks, txt_ids, txt_attn_masks = None, None, None, None
        if 'img' in infer_mode:
            img = batch['image_0'] if 'image_0' in batch else batch['image']
            img_attn_masks = torch.ones([img.size(0), transformer.patch_embed.num_patches + 1], dtype=torch.int64,
                                        device=img.device)
        if 'txt' in infer_mode:
            txt_ids, txt_attn_masks = batch['text_ids'], batch['text_mask']

        def score_fn(co_feats, _):
            T = transformer.max_text_len
            txt_feats, img_feats = (co_feats[:, :T], co_feats[:, T:]) if txt_ids is not None else (None, co_feats)
            out = {'txt_feats': txt_feats, 'img_feats': img_feats, 'co_feats': co_feats,
                   'cls_feats': transformer.pooler(co_feats), 'img_masks': img_attn_masks, 'img_bool_masked_pos': None,
                   'txt_labels': None, 'txt_ids': txt_ids, 'txt_masks': txt_attn_masks}
            return self.itm_head(out['cls_feats'])[:, 1].sum() if target == 'itm' else target(out)

        kw = dict(img=img, txt=txt_ids, img_attn_masks=img_attn_masks, txt_attn_masks=txt_attn_masks)
        return kw, (score_fn if need_score else None)

    def attention_relevance(self, batch, infer_mode='img-txt', layers=None, target='itm', queries=None, method='gradcam'):
        """Relevance of every token for the query tokens, aggregated over the depth, of the backbone pass
        ``infer(batch, infer_mode)`` runs -> fp32 [B, nq, N] (VLMO.attention_relevance: methods, ``layers``, ``queries``
        over the concatenated tokens, eval mode only).  method='gradcam' takes ``target`` as attention_gradcam does;
        method='rollout' runs forward only and ignores it.  Masks and inputs are picked exactly as infer picks them."""
        attnmap.method_weights(method)
        kw, score_fn = self._gradcam_inputs('attention_relevance', batch, infer_mode, target, method == 'gradcam')
        return self.transformer.attention_relevance(score_fn, layers=layers, queries=queries, method=method, **kw)

    # ------------------------------------------------- merged backbone passes
    @staticmethod
    def _split_infer(out, sizes):
        """Cut the batch dimension of one infer() result into consecutive pieces of the given sizes."""
        parts, b0 = [], 0
        for n in sizes:
            parts.append({k: (v[b0:b0 + n] if torch.is_tensor(v) and v.dim() > 0 else v) for k, v in out.items()})
            b0 += n
        return parts

    def _forward_merged(self, batch):
        """The same objectives as forward(), with the backbone passes that share a mode batched into ONE pass each
        (SURVEY 8f-1): V = [ITC image | MIM masked image], L = ITC text, VL = [MLM | ITM positive | ITM negatives].
        Every sample goes through exactly the arithmetic of its own pass (rows are independent: LayerNorm per token,
        attention per sequence), so the results equal the pass-by-pass ones except for the dropout streams; 3
        launches of the 12/24-block stack instead of 7 halve the host time per step."""
        ret = dict()
        names = self.loss_names
        B = batch['image'].size(0)
        dev = batch['image'].device
        if 'mim' in names:
            with torch.no_grad():
                batch['image_bool_masked_pos'] = batch['image_bool_masked_pos'].flatten(1).to(torch.bool)
        # ---- V and L passes as ONE pass of unfused (image, text) pairs: forward_features with fusion_layer = depth runs the
        # image tokens through the 'v' experts and the text tokens through the 'l' experts of EVERY block and never joins them
        # (vlmo.py:400-413 with an empty 'vl' range), i.e. exactly the image-only and text-only passes side by side.  The
        # text-only pass of B sequences alone is ~300 launches of 2 048-row kernels; riding with the 2B images it costs its rows.
        # Pairs: (ITC image_i, text_i), (MIM masked image_i, text_i again -- its text half is discarded, no gradient enters it).
        unfused = ('itc' in names and 'mim' in names and self.transformer_m is None
                   and getattr(self.config.train, 'merge_unfused', True))
        if unfused:
            tr = self.transformer
            T, depth = tr.max_text_len, len(tr.blocks)
            bmp = batch['image_bool_masked_pos']
            img2 = torch.cat([batch['image'], batch['image']], 0)
            bmp2 = torch.cat([torch.zeros_like(bmp), bmp], 0)
            ids2 = torch.cat([batch['text_ids'], batch['text_ids']], 0)
            tm2 = torch.cat([batch['text_mask'], batch['text_mask']], 0)
            ones = torch.ones([2 * B, tr.patch_embed.num_patches + 1], dtype=torch.int64, device=dev)
            lens, _ = self._text_lens(batch)
            co, _ = tr.forward_features(img=img2, txt=ids2, img_attn_masks=ones, txt_attn_masks=tm2, bool_masked_pos=bmp2,
                                        fusion_layer=depth, txt_lens=lens + lens if lens is not None else None)
            img_itc, img_mim, txt_itc = co[:B, T:], co[B:, T:], co[:B, :T]
            batch['_itc_img_infer'] = {'txt_feats': None, 'img_feats': img_itc, 'co_feats': img_itc, 'cls_feats': None,
                                       'img_masks': ones[:B], 'img_bool_masked_pos': None, 'txt_labels': None,
                                       'txt_ids': None, 'txt_masks': None}
            batch['_mim_infer'] = {'txt_feats': None, 'img_feats': img_mim, 'co_feats': img_mim, 'cls_feats': None,
                                   'img_masks': ones[B:], 'img_bool_masked_pos': bmp, 'txt_labels': None,
                                   'txt_ids': None, 'txt_masks': None}
            batch['_itc_txt_infer'] = {'txt_feats': txt_itc, 'img_feats': None, 'co_feats': txt_itc, 'cls_feats': None,
                                       'img_masks': None, 'img_bool_masked_pos': None, 'txt_labels': None,
                                       'txt_ids': batch['text_ids'], 'txt_masks': batch['text_mask']}
        # ---- V pass
        v_parts = []
        if 'itc' in names and not unfused:
            v_parts.append('itc')
        if 'mim' in names and not unfused:
            v_parts.append('mim')
        if v_parts:
            nb = len(v_parts)
            bmp = batch['image_bool_masked_pos'] if 'mim' in names else None
            vb = {'image': torch.cat([batch['image']] * nb, 0) if nb > 1 else batch['image']}
            if bmp is not None:
                zeros = torch.zeros_like(bmp)
                vb['image_bool_masked_pos'] = torch.cat([zeros if p == 'itc' else bmp for p in v_parts], 0)
            out = self.infer(vb, infer_mode='img_only', mask_img=bmp is not None)
            for p, piece in zip(v_parts, self._split_infer(out, [B] * nb)):
                if p == 'itc':
                    piece['img_bool_masked_pos'] = None
                    batch['_itc_img_infer'] = piece
                else:
                    batch['_mim_infer'] = piece
        # ---- L pass, then ITC (its similarities drive the ITM hard negatives)
        if 'itc' in names:
            if not unfused:
                batch['_itc_txt_infer'] = self.infer(batch, infer_mode='txt_only')
            ret.update(objectives.compute_itc(self, batch))
        # ---- VL pass
        vl_parts, ids, masks, imgs = [], [], [], []
        # variable-length text: the parts' lengths side by side; the texts of the ITM negatives that are gathered on the
        # device have no host length and count the full width
        lens, _ = self._text_lens(batch)
        part_lens = []
        if 'mlm' in names:
            vl_parts.append(('mlm', B))
            part_lens.append(lens)
            ids.append(batch['text_ids_mlm'])
            masks.append(batch['text_mask'])
            imgs.append(batch['image'])
        if 'itm' in names:
            img_neg_idx, txt_neg_idx = objectives.sample_itm_negatives(batch, ret if 'itc' in names else None)
            neg = objectives.itm_negative_batch(batch, img_neg_idx, txt_neg_idx)
            vl_parts += [('itm_pos', B), ('itm_neg', 2 * B)]
            part_lens += [lens, neg.get('_txt_lens')]
            ids += [batch['text_ids'], neg['text_ids']]
            masks += [batch['text_mask'], neg['text_mask']]
            imgs += [batch['image'], neg['image']]
        if vl_parts:
            vb = {'text_ids': torch.cat(ids, 0), 'text_mask': torch.cat(masks, 0), 'image': torch.cat(imgs, 0)}
            if lens is not None and all(pl is not None for pl in part_lens):
                vb['_txt_lens'] = tuple(n for pl in part_lens for n in pl)
            out = self.infer(vb, infer_mode='img-txt')
            pieces = dict(zip([p for p, _ in vl_parts], self._split_infer(out, [n for _, n in vl_parts])))
            if 'mlm' in pieces:
                pieces['mlm']['txt_labels'] = batch['text_labels_mlm']
                batch['_mlm_infer'] = pieces['mlm']
            if 'itm_pos' in pieces:
                batch['_itm_infer'] = (pieces['itm_pos'], pieces['itm_neg'])
        if 'mlm' in names:
            ret.update(objectives.compute_mlm(self, batch))
        if 'mim' in names:
            ret.update(objectives.compute_mim(self, batch))
        if 'itm' in names:
            ret.update(objectives.compute_itm(self, batch, ret if 'itc' in names else None))
        return ret

    def forward(self, batch):
        """vlmo_module.py:395-436.  ``config.train.merge_passes = True`` (not a reference option) batches the
        backbone passes of the objectives by mode -- see _forward_merged."""
        batch = defaultdict(lambda: None, batch)
        ret = dict()
        if len(self.loss_names) == 0:
            ret.update(self.infer(batch))
            return ret
        # the VQA pass is not part of the merged passes: with 'vqa' among the losses every objective runs pass by pass
        if (getattr(self.config.train, 'merge_passes', False) and batch['image'] is not None
                and batch['text_ids'] is not None and getattr(self.config.train, 'mim_head_pos', 'img') == 'img'
                and 'vqa' not in self.loss_names):
            return self._forward_merged(batch)
        if 'mlm' in self.loss_names:
            ret.update(objectives.compute_mlm(self, batch))
        if 'mim' in self.loss_names:
            ret.update(objectives.compute_mim(self, batch))
        if 'itc' in self.loss_names:
            ret.update(objectives.compute_itc(self, batch))
        if 'itm' in self.loss_names:
            itc_ret = ret if 'itc' in self.loss_names else None
            ret.update(objectives.compute_itm(self, batch, itc_ret))
        if 'vqa' in self.loss_names:
            ret.update(objectives.compute_vqa(self, batch))
        return ret

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'itc_temp', 'transformer.pos_embed', 'transformer.img_cls_token'}
