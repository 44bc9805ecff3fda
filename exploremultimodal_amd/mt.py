"""Launch tables of the multi-tensor kernels (``vlmo_mt_grad_norm``, ``vlmo_mt_adam``, ``vlmo_mt_ema``,
``vlmo_mt_adam_ema``): the one place that knows how a ``VlmoTensorList`` (include/vlmo_hip.h) is laid out in memory.

A table is built from integers -- addresses and element counts -- so a caller may describe whole tensors
(``optim.FusedAdam``, ``ema.ModelEma``) or slices inside flat buffers (``zero.ZeroAdam``).  A wrong address here is a
kernel writing wherever it points, so nothing outside this module computes a field of the struct."""
import torch

from . import hip

CHUNK = 1 << 16        # elements per workgroup of the multi-tensor kernels


def chunks(numel):
    """(chunk_tensor, chunk_start): one entry per workgroup, tensor t cut at multiples of CHUNK.  A tensor of 0 elements
    gets no chunk."""
    chunk_tensor, chunk_start = [], []
    for t, n in enumerate(numel):
        for off in range(0, n, CHUNK):
            chunk_tensor.append(t)
            chunk_start.append(off)
    return chunk_tensor, chunk_start


class Table:
    """The buffers of one launch on ``dev`` (the object keeps them alive) and ``tl``, the ``hip.TensorList`` over them.

    ``p``, ``g``, ``numel``: one integer per tensor.  With ``m`` and ``v`` (the Adam moments) the int64 block is
    ``[p | g | m | v | numel | chunk_start]`` and the table also gets ``dev_f`` = fp32 ``[lr | wd]`` (left for the caller to
    fill), the ``partial`` scratch and the zeroed ``ctl`` of ``vlmo_mt_grad_norm``; without them the block is
    ``[p | g | numel | chunk_start]`` and ``tl.m``, ``tl.v``, ``tl.lr``, ``tl.wd`` stay NULL.  ``g`` is the view of the
    block's g column, for a caller whose gradient addresses change between launches.  ``ent``: whatever the caller wants
    kept with the table."""
    __slots__ = ('tl', 'nt', 'n_chunks', 'dev_i', 'dev_c', 'dev_f', 'partial', 'ctl', 'g', 'ent')

    def __init__(self, dev, p, g, numel, m=None, v=None, ent=None):
        nt = len(numel)
        chunk_tensor, chunk_start = chunks(numel)
        adam = m is not None
        cols = [p, g, m, v, numel] if adam else [p, g, numel]
        if any(len(c) != nt for c in cols):       # a short column would shift every address after it
            raise ValueError('mt.Table: every column needs one entry per tensor')
        fields = ('p', 'g', 'm', 'v', 'numel') if adam else ('p', 'g', 'numel')
        self.nt, self.n_chunks, self.ent = nt, len(chunk_tensor), ent
        self.dev_i = torch.tensor([x for c in cols for x in c] + chunk_start, dtype=torch.int64).to(dev)
        self.dev_c = torch.tensor(chunk_tensor, dtype=torch.int32).to(dev)
        self.g = self.dev_i[nt:2 * nt]
        self.dev_f = self.partial = self.ctl = None
        tl = self.tl = hip.TensorList()
        for k, name in enumerate(fields + ('chunk_start',)):
            setattr(tl, name, self.dev_i.data_ptr() + 8 * nt * k)
        tl.chunk_tensor = self.dev_c.data_ptr()
        tl.n_chunks, tl.chunk = self.n_chunks, CHUNK
        if adam:
            self.dev_f = torch.empty(max(2 * nt, 1), dtype=torch.float32, device=dev)
            self.partial = torch.empty(max(self.n_chunks, 1), dtype=torch.float32, device=dev)
            self.ctl = torch.zeros(4, dtype=torch.float32, device=dev)
            tl.lr, tl.wd = self.dev_f.data_ptr(), self.dev_f.data_ptr() + 4 * nt


def adam_args(betas, eps, bias_correction, step, adam_w_mode):
    """``hip.AdamArgs`` of the launch that takes its tensors to optimizer step ``step`` (counted from 1)."""
    a = hip.AdamArgs()
    b1, b2 = betas          # the corrections are taken in double, from the betas as given, and rounded once
    a.beta1, a.beta2, a.eps = b1, b2, eps
    if bias_correction:
        a.inv_bc1, a.inv_bc2 = 1.0 / (1.0 - b1 ** step), 1.0 / (1.0 - b2 ** step)
    else:
        a.inv_bc1 = a.inv_bc2 = 1.0
    a.adam_w_mode = 1 if adam_w_mode else 0
    return a


def recent(cache, sig, make, keep=8):
    """``cache[sig]``, made by ``make()`` on a miss.  The sets of tensors that step together change rarely (frozen or unused
    parameters), so a few tables are kept and the oldest leaves when one more arrives."""
    tab = cache.get(sig)
    if tab is None:
        tab = make()
        if len(cache) >= keep:
            cache.pop(next(iter(cache)))
        cache[sig] = tab
    return tab
