"""Exponential moving average of a model's weights: the reference's ``model_ema`` (conf/config.yaml:140-141,
``model_ema: false``, ``model_ema_decay: 0.9999``; written into checkpoints by utils/utils.py:486-508), whose class is
timm's ``ModelEmaV2``.  ``ModelEma`` has that class's surface -- ``.module``, ``.decay``, ``update(model)``,
``set(model)`` -- and runs the update as ONE multi-tensor HIP launch (``vlmo_mt_ema``) over every floating entry of the
state dict, or folded into the AdamW launch by ``optim.FusedAdam.step(ema=...)`` (``vlmo_mt_adam_ema``).

The rule, on the device and on the host alike, is ``e <- e + w * (p - e)`` with ``w = 1 - decay`` (``torch.lerp``), not
``decay * e + w * p``: the same recurrence in exact arithmetic, but ``e == p`` is an exact fixed point of the first, so
the average of a tensor that never changes (a frozen stage, the dVAE) never drifts.

Two deliberate differences from timm: a tensor that appears under two state-dict keys (the MLM decoder weight tied to the
word embeddings) is averaged once per update, not once per key; and key or shape mismatches between the two state dicts
are refused by name where timm zips the values blindly.

This is the plain weight average only.  The momentum-distilled ITC twin (``vlmo_ema``: ``transformer_m``,
``itc_head_m``) is a different feature and stays refused by ``VlmoModule``."""
import copy
import weakref

import torch

from . import hip, mt


def tensor_list(dev, eps):
    """(VlmoTensorList, the ``mt.Table`` that owns its device buffers) of one ``vlmo_mt_ema`` launch over ``eps = [(average, source)]``,
    contiguous fp32 tensors on ``dev``: p = the averages, g = their sources, cut into chunks of ``mt.CHUNK``."""
    tab = mt.Table(dev, [e.data_ptr() for e, _ in eps], [p.data_ptr() for _, p in eps], [e.numel() for e, _ in eps])
    return tab.tl, tab


def _state_slots(module):
    """{state-dict key: (owning module, '_parameters' | '_buffers', name)} as ``nn.Module.state_dict`` enumerates them."""
    slots = {}
    for prefix, mod in module.named_modules(remove_duplicate=False):
        dot = prefix + '.' if prefix else ''
        for name, t in mod._parameters.items():
            if t is not None:
                slots[dot + name] = (mod, '_parameters', name)
        for name, t in mod._buffers.items():
            if t is not None and name not in mod._non_persistent_buffers_set:
                slots[dot + name] = (mod, '_buffers', name)
    return slots


class ModelEma:
    """``ema = ModelEma(model, decay=0.9999, device=None)``; ``ema.update(model)`` after every optimizer step (or
    ``FusedAdam.step(ema=ema)`` / ``loss_scaler(..., model_ema=ema)``, which fold it into the step); evaluate and
    checkpoint ``ema.module``.  ``decay`` is read at every update, so a caller may schedule it.  ``device``: keep the
    average on another device than the model (the update then copies the model's tensors there first)."""

    def __init__(self, model, decay=0.9999, device=None):
        self.module = copy.deepcopy(model)
        self.module.eval()
        for p in self.module.parameters():
            p.requires_grad_(False)
        self.decay = decay
        self.device = device
        if device is not None:
            self.module.to(device=device)
        self._src = weakref.ref(model)      # the model followed: FusedAdam.step(ema=...) gets no model argument
        self._slots = None                  # where the state-dict entries of both models live: see pairs()
        self._tabs = {}                     # (average, source, numel) addresses -> device tables of one launch

    # ---- pairing ---------------------------------------------------------------------------------------------
    def source(self):
        """The model this average follows: the one given to the constructor or to the latest update() / set()."""
        model = self._src()
        if model is None:
            raise RuntimeError('ModelEma: the model this average follows no longer exists')
        return model

    def pairs(self, model=None, rebuild=False):
        """[(key, average, source)] over the two state dicts, one entry per distinct average tensor (tied weights show
        up under several keys).  Mismatched keys or shapes raise with the offending names.

        Two ``state_dict()`` walks cost milliseconds of host time at Base, every step.  So the walk happens once per model
        object and leaves the SLOTS of the entries (owning module, parameter or buffer, name); later calls read the
        tensors out of the slots, which follows a tensor that is replaced or re-homed (``p.data = ...``, ZeroAdam) but
        not a module that is added or swapped afterwards: ``rebuild=True`` (or ``set()``) walks again."""
        if model is None:
            model = self.source()
        if rebuild or self._slots is None or self._src() is not model:
            self._src = weakref.ref(model)
            esd, msd = self.module.state_dict(), model.state_dict()
            if esd.keys() != msd.keys():
                missing = [k for k in esd if k not in msd]
                extra = [k for k in msd if k not in esd]
                raise KeyError(f'ModelEma: the state dicts do not match: not in the model {missing}, not in the average {extra}')
            es, ms = _state_slots(self.module), _state_slots(model)
            # a module with state-dict hooks or extra state has entries no slot describes: walk every time then
            self._slots = [(k, es[k], ms[k]) for k in esd] if es.keys() == esd.keys() == ms.keys() else False
        if self._slots:
            ents = [(k, getattr(em, ek)[en], getattr(mm, mk)[mn]) for k, (em, ek, en), (mm, mk, mn) in self._slots]
        else:
            esd, msd = self.module.state_dict(), model.state_dict()
            ents = [(k, e, msd[k]) for k, e in esd.items()]
        bad = [f'{k}: average {tuple(e.shape)}, model {tuple(p.shape)}' for k, e, p in ents if e.shape != p.shape]
        if bad:
            raise ValueError(f'ModelEma: shape mismatch for {"; ".join(bad)}')
        out, seen = [], set()
        for ent in ents:
            e = ent[1]
            ident = (e.data_ptr(), e.numel(), e.device) if e.numel() else (id(e),)
            if ident not in seen:
                seen.add(ident)
                out.append(ent)
        return out

    # ---- update ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, model):
        """One step of the average toward ``model``'s current state: floating entries by the rule above, the others
        (integer buffers) copied."""
        self.update_pairs(self.pairs(model), 1.0 - self.decay)

    @torch.no_grad()
    def set(self, model):
        """Make the average an exact copy of ``model``'s state."""
        for _, e, p in self.pairs(model, rebuild=True):
            e.copy_(p)          # (an in-place torch op: it moves the version counter itself)

    def update_pairs(self, pairs, w):
        """The update of the given ``pairs()`` entries (FusedAdam.step(ema=...) passes the ones its own launch did not
        cover).  Device entries go through one ``vlmo_mt_ema`` launch per device, host entries through ``lerp_``."""
        if not 0.0 <= w <= 1.0:
            raise ValueError(f'ModelEma: decay = {1.0 - w} is outside [0, 1]')
        by_dev, host_e, host_p = {}, [], []
        for k, e, p in pairs:
            if p.device != e.device:
                p = p.to(e.device)
            if not e.is_floating_point():
                e.copy_(p)
            elif e.is_cuda:
                if e.dtype != torch.float32 or p.dtype != torch.float32 or not e.is_contiguous() or not p.is_contiguous():
                    raise RuntimeError(f'ModelEma: {k}: device entries must be contiguous fp32 (there is no other kernel)')
                if e.numel():
                    by_dev.setdefault(e.device, []).append((e, p))
            else:
                host_e.append(e)
                host_p.append(p.to(e.dtype))
        for dev, eps in by_dev.items():
            with torch.cuda.device(dev):
                hip.mt_ema(self._table(dev, eps), w)
        if host_e:
            torch._foreach_lerp_(host_e, host_p, w)
        # the kernel wrote behind autograd's back: without this the engine's bf16 weight shadows (engine.ShadowCache,
        # keyed on the version counter) would keep serving the previous average to ema.module's forward
        self.touched([e for _, e, _ in pairs])

    @staticmethod
    def touched(tensors):
        if tensors:
            torch.autograd.graph.increment_version(tensors)

    def _table(self, dev, eps):
        """The launch tables of `eps`.  The addresses are fixed between steps, so they are uploaded once per set of tensors
        (as FusedAdam._tables caches its own)."""
        sig = (dev, tuple((e.data_ptr(), p.data_ptr(), e.numel()) for e, p in eps))
        return mt.recent(self._tabs, sig, lambda: tensor_list(dev, eps))[0]

    # ---- state -----------------------------------------------------------------------------------------------
    def state_dict(self):
        return self.module.state_dict()

    def load_state_dict(self, state_dict, strict=True):
        return self.module.load_state_dict(state_dict, strict=strict)
