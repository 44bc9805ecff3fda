"""Autograd glue between the nn.Module mirror (vlmo.py) and the HIP C-ABI.

Layout ("packed rows"): the token matrix of one backbone pass is [M, d] with
all text tokens of the batch first (B*T rows), then all image tokens (B*P rows).
LayerNorm / linear layers do not care about row order, so below the fusion
layer the shared-weight ops (norm1, qkv, proj, norm2) run ONCE over both
modalities and only the expert FFNs and attention look at row ranges; above it
attention finds a fused sequence through a two-segment descriptor, so the
reference's torch.cat([txt, img], dim=1) (vlmo.py:406) never materialises.

The residual stream is fp32 (as under the reference's autocast), GEMM operands
bf16 with fp32 accumulation, parameters fp32 masters with cached bf16 shadows.
"""
import ctypes
import functools
import os as _os
import sys
from collections import namedtuple

import torch

from . import hip

LN_EPS = 1e-12          # vlmo_module.py:21-23
GRAD_SINK = None         # set by dp.GradReducer: block gradients are accumulated straight into its flat buckets
# Weight-gradient GEMMs + bias column sums on a side stream: '1' always, '0' never, unset = by the rule below.
# The GEMM kernels take whole CUs (128 KB of LDS, every vector register), so two streams time-slice the chip instead of
# sharing it: the overlap pays only where the main stream's kernels leave CUs idle (short kernels, partial dispatch
# rounds).  In-session A/Bs, side stream against one stream, no reducer: VLMo-Base at 64 pairs (16 704 rows per pass)
# 14.70 / 14.66 / 14.66 against 14.63 / 14.64 / 14.64 ms and 14.25 / 14.25 against 14.18 / 14.20 on another box; the
# four-loss objective at 32 pairs (passes of 33 408 and 12 608 rows) 48.1 / 47.9 against 47.3 / 47.3; VLMo-Large at 32
# pairs (8 352 rows) 25.02 / 25.03 against 25.58 / 25.55.  So: one stream for passes of ONE_STREAM_ROWS rows and more, the
# side stream below -- and always under a gradient reducer, where the side stream is what lets a block's gradients
# finish (and their collective start) while the activation gradients of the blocks below are still being computed
# (dp.GradReducer waits on the per-block grad_ready events).
_ov = _os.environ.get('VLMO_OVERLAP_WGRAD')
OVERLAP_WGRAD = None if _ov is None else _ov != '0'
ONE_STREAM_ROWS = 12288


def _use_side_stream(sink, rows):
    if OVERLAP_WGRAD is not None:
        return OVERLAP_WGRAD
    return sink is not None or rows < ONE_STREAM_ROWS


DEFAULT_TILE = -1        # GEMM tile: -1 = chosen per shape by the library (see vlmo_gemm_nt)


class ShadowCache:
    """bf16 copies (W and W^T) of fp32 master weights, refreshed when the
    parameter's version counter changes (optimizer step / load_state_dict)."""

    def __init__(self):
        self._c = {}

    def get(self, p, need_t=True):
        key = id(p)
        ent = self._c.get(key)
        ver = (p._version, p.data_ptr())
        if ent is None or ent[0] != ver or (need_t and ent[2] is None):
            w2 = p.detach().reshape(p.shape[0], -1)
            w = torch.empty(w2.shape, dtype=torch.bfloat16, device=p.device)
            wt = torch.empty((w2.shape[1], w2.shape[0]), dtype=torch.bfloat16, device=p.device) if need_t else None
            hip.cast_weight(w2, w, wt)
            ent = (ver, w, wt)
            self._c[key] = ent
        return ent[1], ent[2]

    def refresh(self, params):
        """Bring the shadows of `params` (2-D weights, W and W^T) up to date in ONE launch: after an optimizer step every
        weight is stale, and one cast launch per weight was 0.65 ms of an 18 ms training step.  Buffers of an unchanged
        shape are overwritten in place (the cast is ordered behind the step's kernels on the caller's stream)."""
        jobs = []
        for p in params:
            key = id(p)
            ent = self._c.get(key)
            ver = (p._version, p.data_ptr())
            if ent is not None and ent[0] == ver and ent[2] is not None:
                continue
            w2 = p.detach().reshape(p.shape[0], -1)
            # in place only when nobody else holds the pair: a graph whose forward ran BEFORE the parameter update keeps its
            # shadows for its input-gradient GEMMs (ctx.keep), and overwriting them would make that backward use the NEW
            # weights (forward A, optimizer step, forward B, backward A).  The cache entry is the only other owner.
            if (ent is not None and ent[1].shape == w2.shape and ent[2] is not None
                    and sys.getrefcount(ent[1]) <= 2 and sys.getrefcount(ent[2]) <= 2):
                w, wt = ent[1], ent[2]
            else:
                w = torch.empty(w2.shape, dtype=torch.bfloat16, device=p.device)
                wt = torch.empty((w2.shape[1], w2.shape[0]), dtype=torch.bfloat16, device=p.device)
            jobs.append((w2, w, wt))
            self._c[key] = (ver, w, wt)
        if jobs:
            hip.cast_weight_multi(jobs)

    def qkv_bias(self, q_bias, v_bias):
        """cat(q_bias, 0, v_bias) (vlmo.py:72-75), cached until either parameter changes."""
        key = ('qkvb', id(q_bias))
        ver = (q_bias._version, v_bias._version, q_bias.data_ptr())
        ent = self._c.get(key)
        if ent is None or ent[0] != ver:
            ent = (ver, torch.cat([q_bias.detach(), torch.zeros_like(q_bias), v_bias.detach()]))
            self._c[key] = ent
        return ent[1]

    def clear(self):
        self._c.clear()


def _seg(a0, la, b0, lb, device):
    """Segment descriptors {rowA, lenA, rowB, lenB} of a launch's sequences, int32 [sequences, 4] on `device`."""
    return torch.stack([a0, la, b0, lb], 1).to(device=device, dtype=torch.int32).contiguous()


class _PlanStatic:
    """Shape-only part of a plan (segment descriptors, row maps): built once per (B, T, P, device).
    Building it copies a few small host tensors to the device, which would stall the host every pass."""
    _cache = {}

    @classmethod
    def get(cls, B, T, P, device):
        key = (B, T, P, str(device))
        st = cls._cache.get(key)
        if st is None:
            st = cls(B, T, P, device)
            cls._cache[key] = st
        return st

    def __init__(self, B, T, P, device):
        nt = B * T
        ar = torch.arange(B, dtype=torch.int32)
        z = torch.zeros(B, dtype=torch.int32)
        tl, pl = torch.full((B,), T, dtype=torch.int32), torch.full((B,), P, dtype=torch.int32)
        self.seg_txt = _seg(ar * T, tl, z, z, device) if T else None
        self.seg_img = _seg(nt + ar * P, pl, z, z, device) if P else None
        self.seg_vl = _seg(ar * T, tl, nt + ar * P, pl, device) if (T and P) else None
        # below the fusion layer text and image sequences attend separately but in ONE launch (longest first:
        # the workgroups of the short text sequences fill the tail of the image ones)
        self.seg_sep = torch.cat([self.seg_img, self.seg_txt]).contiguous() if (T and P) else None
        # packed row -> row of the [B, T+P, d] output (text first, vlmo.py:406)
        N = T + P
        rm_t = (torch.arange(B).view(B, 1) * N + torch.arange(T).view(1, T)).reshape(-1)
        rm_i = (torch.arange(B).view(B, 1) * N + T + torch.arange(P).view(1, P)).reshape(-1)
        self.rowmap = torch.cat([rm_t, rm_i]).to(torch.int32).to(device)
        # drop-path group of every packed row: text rows of sample b -> b, image rows -> B + b (a per-sample
        # scale vector [2B] is expanded inside the kernels through this map)
        self.row_group = torch.cat([torch.arange(B).repeat_interleave(T),
                                    B + torch.arange(B).repeat_interleave(P)]).to(torch.int32).to(device)


def check_txt_lens(txt_lens, B, T):
    """The row counts of a variable-length text batch as a tuple of B python ints, each in [1, T] (host only: no
    device is asked).  A sequence of ints or a CPU integer tensor is taken; a wrong count, a value outside [1, T], a
    non-integer or a device tensor raises ValueError."""
    if torch.is_tensor(txt_lens):
        if txt_lens.device.type != 'cpu':
            raise ValueError('txt_lens must live on the host (python ints or a CPU tensor): reading a device tensor '
                             'would stall the pass (objectives.attach_text_lens builds it from the host batch)')
        if txt_lens.dim() != 1 or txt_lens.dtype.is_floating_point or txt_lens.dtype in (torch.bool, torch.complex64,
                                                                                          torch.complex128):
            raise ValueError(f'txt_lens must be a 1-D integer tensor, got {txt_lens.dtype} {tuple(txt_lens.shape)}')
        txt_lens = txt_lens.tolist()
    try:
        lens = tuple(txt_lens)
    except TypeError:
        raise ValueError(f'txt_lens must be a sequence of {B} ints, got {type(txt_lens).__name__}') from None
    if len(lens) != B:
        raise ValueError(f'txt_lens has {len(lens)} entries for a batch of {B}')
    for n in lens:
        if isinstance(n, bool) or not isinstance(n, int):
            raise ValueError(f'txt_lens must hold python ints, got {n!r}')
        if not 1 <= n <= T:
            raise ValueError(f'txt_lens entries must be in [1, {T}], got {n}')
    return lens


class _PlanRagged:
    """Shape-only part of a plan whose text sample b keeps its first lens[b] positions (1 <= lens[b] <= T) as packed
    rows off[b] .. off[b + 1]; the image rows start at nt = sum(lens).  The tables are functions of the host lengths
    alone.  They are built with device ops whose sizes come from the host, out of ONE small device tensor (off, int32
    [B + 1]: the caller's, or uploaded here from pinned memory without waiting), so building asks the device nothing;
    the last few are kept, so the passes of a step that share a batch share its tables."""
    _cache = {}
    KEEP = 8

    @classmethod
    def get(cls, B, T, P, device, lens, off=None):
        key = (B, T, P, str(device), lens)
        st = cls._cache.pop(key, None)
        if st is None:
            st = cls(B, T, P, device, lens, off)
            while len(cls._cache) >= cls.KEEP:
                cls._cache.pop(next(iter(cls._cache)))
        cls._cache[key] = st                      # most recently used last
        return st

    def __init__(self, B, T, P, device, lens, off=None):
        dev = torch.device(device)
        host_off = [0]
        for n in lens:
            host_off.append(host_off[-1] + n)
        nt = self.nt = host_off[-1]
        self.maxT = max(lens)
        if off is None:
            off = torch.tensor(host_off, dtype=torch.int32)
            if dev.type != 'cpu':
                off = off.pin_memory().to(dev, non_blocking=True)
        elif off.device != dev or off.dtype != torch.int32 or tuple(off.shape) != (B + 1,):
            raise ValueError(f'txt_off must be an int32 [{B + 1}] tensor on {dev}')
        self.off = off
        i32 = torch.int32
        ar = torch.arange(B, dtype=i32, device=dev)
        z = torch.zeros(B, dtype=i32, device=dev)
        row0, ln = off[:-1], off[1:] - off[:-1]
        pl = torch.full((B,), P, dtype=i32, device=dev)
        img0 = nt + ar * P
        self.seg_txt = _seg(row0, ln, z, z, dev)
        self.seg_img = _seg(img0, pl, z, z, dev) if P else None
        self.seg_vl = _seg(row0, ln, img0, pl, dev) if P else None
        self.seg_sep = torch.cat([self.seg_img, self.seg_txt]).contiguous() if P else None
        # sample and in-sequence position of every packed text row
        rb = torch.repeat_interleave(torch.arange(B, device=dev), ln.long(), output_size=nt)
        tt = torch.arange(nt, device=dev) - row0.long()[rb]
        self.src = (rb * T + tt).to(i32)          # packed text row -> b * T + t: ids, key mask (vlmo_embed_txt_rows_fwd)
        N = T + P
        bi = torch.arange(B, device=dev).repeat_interleave(P)
        rm_i = bi * N + T + torch.arange(P, device=dev).repeat(B)
        self.rowmap = torch.cat([rb * N + tt, rm_i]).to(i32)
        self.row_group = torch.cat([rb, B + bi]).to(i32)


class Plan:
    """Row layout + attention launches of one backbone pass.

    txt_lens (a tuple from check_txt_lens): text sample b has its first txt_lens[b] positions only; nt = sum(txt_lens),
    the segment descriptors, the row map into [B, T + P, d], the drop-path groups and the key mask are those of the
    packed rows, and maxT is the longest text (T without lengths).  T stays the width of the id matrix and of the
    output.  txt_off: the prefix sums of txt_lens as an int32 [B + 1] tensor already on the device (optional)."""

    def __init__(self, B, T, P, device, txt_mask=None, img_mask=None, txt_lens=None, txt_off=None):
        self.B, self.T, self.P = B, T, P
        self.device = device
        self.txt_lens = txt_lens
        if txt_lens is not None:
            assert T > 0
            st = _PlanRagged.get(B, T, P, device, txt_lens, txt_off)
            self.nt, self.maxT, self.txt_src, self.txt_off = st.nt, st.maxT, st.src, st.off
        else:
            st = _PlanStatic.get(B, T, P, device)
            self.nt, self.maxT = B * T, T
        self.ni = B * P
        self.M = self.nt + self.ni
        self.seg_txt, self.seg_img, self.seg_vl, self.seg_sep = st.seg_txt, st.seg_img, st.seg_vl, st.seg_sep
        self.rowmap, self.row_group = st.rowmap, st.row_group
        # key-padding mask over packed rows (vlmo.py:89-91); None = all valid.  A missing mask counts as all ones (an
        # empty one when the pass has no such rows); with text lengths the text part keeps the packed positions only
        # (st.src: packed text row -> element of the [B, T] mask).
        self.keymask = None
        if txt_mask is not None or img_mask is not None:
            txt, img = (m.reshape(-1).to(torch.int32) if n and m is not None else torch.ones(n, dtype=torch.int32, device=device)
                        for n, m in ((B * T, txt_mask), (self.ni, img_mask)))
            self.keymask = torch.cat([txt if txt_lens is None else txt[st.src.long()], img]).contiguous()

    def attn_launches(self, fused):
        # the maximum a launch reports picks its attention kernel: with text lengths it is the batch's true maximum
        if fused and self.seg_vl is not None:
            return [(self.seg_vl, self.B, self.maxT + self.P)]
        if self.seg_sep is not None:
            return [(self.seg_sep, 2 * self.B, max(self.maxT, self.P))]
        out = []
        if self.seg_txt is not None:
            out.append((self.seg_txt, self.B, self.maxT))
        if self.seg_img is not None:
            out.append((self.seg_img, self.B, self.P))
        return out


class BlockMeta:
    """Static (non-tensor) description of one Block call."""

    def __init__(self, plan, heads, d, hidden, fused, expert_ranges, training, drop, attn_drop,
                 row_scale1, row_scale2, seed, eps=LN_EPS):
        self.plan, self.heads, self.d, self.hidden = plan, heads, d, hidden
        self.eps = eps
        self.fused = fused
        self.expert_ranges = expert_ranges      # [(row0, nrows)], one per expert in param order
        self.training = training
        self.drop = hip.drop_params(drop, training)
        self.attn_drop = hip.drop_params(attn_drop, training)
        self.rs1, self.rs2 = row_scale1, row_scale2
        self.seed = seed
        self.shadows = None
        self.tile = DEFAULT_TILE
        # opt-in: capture(qkv, dctx, plan, fused), run by StackFn.backward after vlmo_stack_bwd on the same stream with
        # views of this block's saved bf16 qkv rows [M, 3d] and of its bf16 dctx [M, d] (see _run_captures)
        self.capture = None


_SIDE = {}


def _side_stream(dev):
    """The weight-gradient stream of a device: lowest dispatch priority, so the activation-gradient chain
    on the caller's stream (the critical path) wins every freed compute-unit slot."""
    s = _SIDE.get(dev)
    if s is None:
        make = lambda: torch.cuda.ExternalStream(hip.side_stream_create(True), device=dev)
        with torch.cuda.device(dev):
            s = pick_stream(dev, make, [torch.cuda.current_stream(dev)])
        _SIDE[dev] = s
    return s


_PROBE_SCRATCH = {}


def _queued_behind(dev, busy, cand):
    """True when work on stream `cand` waits for kernels on stream `busy` (the two share a hardware queue, or their
    queues share a command-processor pipe): a long memory-bound kernel sequence goes to `busy`, a one-element kernel
    to `cand` right behind it; sharing shows as the small kernel finishing only when the long ones have."""
    # one 64 MB scratch per device, kept: a probe per rank and candidate at start-up must not allocate 256 MB each time
    # (8 ranks x up to 16 probes); 24 passes of ~25 us keep `busy` occupied for the same ~0.6 ms
    scratch = _PROBE_SCRATCH.get(dev)
    if scratch is None:
        scratch = _PROBE_SCRATCH[dev] = torch.empty(1 << 24, device=dev)
    tiny = torch.empty(64, device=dev)
    votes = 0
    for _ in range(2):
        torch.cuda.synchronize(dev)
        t0, t1, t2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        with torch.cuda.stream(busy):
            scratch.zero_()                                     # the timer starts once `busy` is running
            t0.record()
            for _ in range(24):
                scratch.mul_(1.0)
            t1.record()
        with torch.cuda.stream(cand):
            tiny.zero_()
            t2.record()
        torch.cuda.synchronize(dev)
        votes += t0.elapsed_time(t2) > 0.5 * t0.elapsed_time(t1)
    return votes == 2


def pick_stream(dev, make, against, tries=8):
    """A stream from make() whose work does not queue behind any stream of `against`.  HIP hands streams their
    hardware queues round-robin and the queues are spread over the command processor's pipes by creation order, so
    whether two streams can run side by side depends on what else (RCCL, the framework) created streams before:
    measured here, a step with the reducer took 22.9 instead of 16.5 ms when the communication stream's queue shared the
    main stream's pipe (rocprofv3: every kernel on it started ~50 us late), and one stream in four of a fresh batch
    finishes a one-element kernel 1.4 ms late behind a busy main stream (tools/pipe_probe.py).  Probing is the only
    portable way to know.  Falls back to the first candidate when every one collides."""
    first = None
    for _ in range(tries):
        s = make()
        first = first or s
        with torch.cuda.stream(s):
            torch.zeros(1, device=dev)                          # binds the hardware queue
        if not any(_queued_behind(dev, a, s) for a in against):
            return s
    import warnings
    warnings.warn('no stream found that runs beside the main stream: side-stream work will serialise')
    return first


# ---- the per-block parameter order -------------------------------------------------------------------------------
# vlmo.Block._params is its single producer: N_SHARED tensors every row of the block uses (gamma_1, gamma_2, norm1 w / b,
# qkv_w, q_bias, v_bias, proj_w, proj_b, norm2 w / b), then N_EXPERT per expert FFN of the call (fc1_w, fc1_b, fc2_w,
# fc2_b).  The shared tensors and each expert are one parameter GROUP: one flat gradient bucket, one reducer bucket, one
# unit of in-place accumulation.  Everything below that needs the order goes through block_groups().
N_SHARED, N_EXPERT = 11, 4
QKV_W, PROJ_W = 4, 7            # the weight matrices inside the shared group
FC1_W, FC2_W = 0, 2             # ... and inside an expert group
ARENA_EXPERTS = 3               # experts a block can own (v, l, vl): the room of its reducer arena

Group = namedtuple('Group', 'params lo hi')     # params == tuple(block parameter list[lo:hi]); lo == 0: the shared group


def block_groups(bp):
    """One block's parameter list (per-block order) as its groups: the shared group, then one per expert."""
    nexp, rest = divmod(len(bp) - N_SHARED, N_EXPERT)
    if nexp < 1 or rest:
        raise ValueError(f'{len(bp)} tensors are not a block parameter list ({N_SHARED} shared + {N_EXPERT} per expert)')
    cuts = [0] + [N_SHARED + N_EXPERT * e for e in range(nexp + 1)]
    return [Group(tuple(bp[lo:hi]), lo, hi) for lo, hi in zip(cuts, cuts[1:])]


# ---- the buffers behind a VlmoBlockDesc's pointers ----------------------------------------------------------------
# Each layout is declared HERE and nowhere else; sizes, pointers and views are derived (_layouts).  Widths are named:
# 'd', '3d', 'hid' (the FFN width, BlockMeta.hidden) and '1'.
# Row tables, (descriptor field, columns): a buffer of M rows holds field after field, each an [M, columns] matrix.
#   the saved activations of one block, bf16 ...
SLAB_BF16 = (('y1', 'd'), ('qkv', '3d'), ('ctx', 'd'), ('zd1', 'd'), ('y2', 'd'), ('u', 'hid'), ('h', 'hid'), ('zd2', 'd'))
#   ... and fp32, followed by the log-sum-exp rows of the block's attention launches (_lse_layout)
SLAB_F32 = (('x1', 'd'), ('mean1', '1'), ('rstd1', '1'), ('mean2', '1'), ('rstd2', '1'))
#   one set of the rotating backward temporaries, bf16; '=f': the field shares the matrix of field f (_run_captures
#   says why dctx may live in dy2)
TEMPS_BF16 = (('dz2', 'd'), ('du', 'hid'), ('dy2', 'd'), ('dctx', '=dy2'), ('dz1', 'd'), ('dqkv', '3d'), ('dy1', 'd'))
# Bucket tables, (descriptor field, shape, parameter): the flat fp32 gradient bucket of a parameter group holds tensor
# after tensor; parameter = index in the group (per-block order) of the parameter whose gradient the tensor is.  A
# field of None continues the buffer of the field before it: dqkv_b is [3d] = q_bias | k (constant zero: no parameter)
# | v_bias.
SHARED_GRADS = (('dg1', ('d',), 0), ('dg2', ('d',), 1), ('dn1w', ('d',), 2), ('dn1b', ('d',), 3), ('dn2w', ('d',), 9),
                ('dn2b', ('d',), 10), ('dqkv_w', ('3d', 'd'), QKV_W), ('dproj_w', ('d', 'd'), PROJ_W), ('dproj_b', ('d',), 8),
                ('dqkv_b', ('d',), 5), (None, ('d',), None), (None, ('d',), 6))
EXPERT_GRADS = (('dw1', ('hid', 'd'), FC1_W), ('db1', ('hid',), 1), ('dw2', ('d', 'hid'), FC2_W), ('db2', ('d',), 3))


class _Rows:
    """A row table at one (d, hid): at = {field: (first column, columns)}, cols = the columns of a whole row.  In a
    buffer of M rows the field is the [M, columns] matrix that starts at element M * first column."""

    def __init__(self, table, width):
        self.at, self.cols = {}, 0
        for name, w in table:
            self.at[name] = self.at[w[1:]] if w[0] == '=' else (self.cols, width[w])
            self.cols = max(self.cols, sum(self.at[name]))      # a shared matrix ends inside the row: no new columns

    def wire(self, D, base, M, itemsize):
        """The descriptor pointers of a buffer of M rows at address `base`."""
        for name, (c0, _) in self.at.items():
            setattr(D, name, base + c0 * M * itemsize)

    def view(self, buf, i, M, name):
        """Field `name` of the i-th M-row buffer of the flat tensor `buf` (buffer after buffer), as [M, columns]."""
        c0, n = self.at[name]
        return buf[(i * self.cols + c0) * M:(i * self.cols + c0 + n) * M].view(M, n)


class _Bucket:
    """A bucket table at one (d, hid): entries = ((field, shape, offset, numel, parameter), ...), numel of the whole
    bucket, and vectors = ((lo, hi), ...), the maximal runs of 1-D tensors (the column folds ACCUMULATE into those)."""

    def __init__(self, table, width):
        ent, vec, off = [], [], 0
        for field, shape, par in table:
            shape = tuple(width[w] for w in shape)
            n = shape[0] * (shape[1] if len(shape) > 1 else 1)
            ent.append((field, shape, off, n, par))
            if len(shape) == 1:
                lo = vec.pop()[0] if vec and vec[-1][1] == off else off     # extends the run that ends here
                vec.append((lo, off + n))
            off += n
        self.entries, self.vectors, self.numel = tuple(ent), tuple(vec), off


_Layouts = namedtuple('_Layouts', 'slab f32 temps buckets')


@functools.lru_cache(maxsize=None)
def _layouts(d, hid):
    """The tables above as plain integers, resolved once per (d, hid); buckets[is_expert] = the group kind's bucket."""
    width = {'1': 1, 'd': d, '3d': 3 * d, 'hid': hid}
    return _Layouts(_Rows(SLAB_BF16, width), _Rows(SLAB_F32, width), _Rows(TEMPS_BF16, width),
                    (_Bucket(SHARED_GRADS, width), _Bucket(EXPERT_GRADS, width)))


def _lse_layout(launches, heads):
    """[(row stride, elements)] of the fp32 log-sum-exp buffers of a block's attention launches (Plan.attn_launches): one
    row of ceil32(longest sequence) per (sequence, head)."""
    strides = [((ml + 31) // 32) * 32 for _, _, ml in launches]
    return [(s, nseq * heads * s) for s, (_, nseq, _) in zip(strides, launches)]


def group_numel(g, d, hid):
    """Elements of the group's flat gradient bucket (what _fill_grads carves; the shared one includes the k-bias hole)."""
    return _layouts(d, hid).buckets[g.lo > 0].numel


def group_layout(g, d, hid):
    """[(parameter, offset)] of the group inside its flat gradient bucket, in bucket order."""
    return [(g.params[par], off) for _, _, off, _, par in _layouts(d, hid).buckets[g.lo > 0].entries if par is not None]


def _wire_slabs(D, pb, pf, M, d, hid, heads, launches):
    """Saved-activation pointers and attention launches of a VlmoBlockDesc: the bf16 slab at address pb, the fp32 slab
    at pf with the launches' log-sum-exp buffers behind its rows."""
    L = _layouts(d, hid)
    L.slab.wire(D, pb, M, 2)
    L.f32.wire(D, pf, M, 4)
    off = pf + L.f32.cols * M * 4
    D.n_attn = len(launches)
    for i, ((seg, nseq, ml), (stride, n)) in enumerate(zip(launches, _lse_layout(launches, heads))):
        D.seg[i], D.nseq[i], D.maxlen[i] = seg.data_ptr(), nseq, ml
        D.lse_stride[i], D.lse[i] = stride, off
        D.attn_seed_idx[i], D.attn_seq0[i] = i, 0
        off += n * 4


def _fill_forward(D, meta, groups, launches, M, pb, pf, need_bwd, keep):
    """Forward part of a VlmoBlockDesc: geometry, parameters (fp32 vectors, bf16 weight shadows) and the saved-
    activation slabs at pb (bf16) / pf (fp32).  groups: block_groups() of the block's parameters; x / x2 are set by
    the caller."""
    (g1, g2, n1w, n1b, qkv_w, q_bias, v_bias, proj_w, proj_b, n2w, n2b) = groups[0].params
    nexp = len(meta.expert_ranges)
    pl, d, H, hid = meta.plan, meta.d, meta.heads, meta.hidden
    sh = meta.shadows
    qkv_bias = sh.qkv_bias(q_bias, v_bias)
    D.M, D.d, D.hidden, D.heads = M, d, hid, H
    D.n_experts = nexp
    for i, (r0, n) in enumerate(meta.expert_ranges):
        D.exp_row0[i], D.exp_rows[i] = r0, n
    _wire_slabs(D, pb, pf, M, d, hid, H, launches)
    D.keymask = hip._p(pl.keymask)
    D.eps = meta.eps
    D.drop_thresh, D.inv_keep = meta.drop
    D.attn_drop_thresh, D.attn_inv_keep = meta.attn_drop
    D.seed = meta.seed & 0xFFFFFFFFFFFFFFFF
    D.rs1, D.rs2 = hip._p(meta.rs1), hip._p(meta.rs2)
    D.row_index = pl.row_group.data_ptr() if meta.rs1 is not None else None
    D.tile, D.need_bwd = meta.tile, int(need_bwd)
    D.g1, D.g2, D.n1w, D.n1b, D.n2w, D.n2b = (t.data_ptr() for t in (g1, g2, n1w, n1b, n2w, n2b))
    D.qkv_bias, D.proj_b = qkv_bias.data_ptr(), proj_b.data_ptr()
    (a, at), (c, ct) = sh.get(qkv_w), sh.get(proj_w)
    D.qkv_w, D.qkv_wT, D.proj_w, D.proj_wT = a.data_ptr(), at.data_ptr(), c.data_ptr(), ct.data_ptr()
    keep += [qkv_bias, a, at, c, ct]
    for i, g in enumerate(groups[1:]):
        w1, b1, w2, b2 = g.params
        a, at = sh.get(w1)
        c, ct = sh.get(w2)
        D.w1[i], D.w1T[i], D.w2[i], D.w2T[i] = a.data_ptr(), at.data_ptr(), c.data_ptr(), ct.data_ptr()
        D.b1[i], D.b2[i] = b1.data_ptr(), b2.data_ptr()
        keep += [a, at, c, ct]


SPLIT_BWD_ATTENTION = _os.environ.get('VLMO_SPLIT_BWD_ATTN', '1') != '0'


def _split_backward_attention(D, meta):
    """Below the fusion layer the image and the text sequences share ONE forward attention launch (Plan.seg_sep, image
    sequences first).  The single-pass backward sizes a workgroup (one wave per key tile, LDS images) for the launch's
    LONGEST sequence, so in the shared launch every 64-token text sequence would hold a whole CU with 2 of 7 waves
    working (122 us for the pair at Base B=64); as two launches the text one takes 34 KB of LDS and 128 threads per
    workgroup, four to a CU (79 + 16 us).  The forward's log-sum-exp buffer is addressed per sequence with the shared
    launch's stride, so the two backward launches are views of it."""
    pl = meta.plan
    if (not SPLIT_BWD_ATTENTION or meta.fused or D.n_attn != 1 or pl.seg_sep is None or not (pl.T and pl.P)
            or D.nseq[0] != 2 * pl.B or max(pl.T, pl.P) > 256):
        return
    stride = D.lse_stride[0]
    D.n_attn = 2
    D.nseq[0], D.nseq[1] = pl.B, pl.B
    D.maxlen[0], D.maxlen[1] = pl.P, pl.maxT                             # the text launch's true maximum
    D.lse_stride[1] = stride
    D.seg[1] = D.seg[0] + pl.B * 16                                       # 4 int32 per sequence
    # the text launch regenerates the attention-dropout mask of ITS sequences of the shared forward launch
    # (sequences [B, 2B) under the forward's seed), not the mask of a second forward launch
    D.attn_seed_idx[1], D.attn_seq0[1] = D.attn_seed_idx[0], pl.B
    D.lse[1] = D.lse[0] + pl.B * meta.heads * stride * 4


def _fill_grads(D, flats, d, hid, nexp):
    """Parameter-gradient pointers of a VlmoBlockDesc from flat fp32 storage (flats[0]: shared parameters,
    flats[1 + e]: expert e) -> gradient tensors in per-block parameter order."""
    buckets = _layouts(d, hid).buckets
    grads = [None] * (N_SHARED + N_EXPERT * nexp)
    for gi, flat in enumerate(flats[:1 + nexp]):
        p0 = flat.data_ptr()
        first = N_SHARED + N_EXPERT * (gi - 1) if gi else 0         # the group's first parameter in per-block order
        for field, shape, off, n, par in buckets[gi > 0].entries:
            if field is not None and gi:
                getattr(D, field)[gi - 1] = p0 + off * 4
            elif field is not None:
                setattr(D, field, p0 + off * 4)
            if par is not None:
                grads[first + par] = flat[off:off + n].view(shape)
    return grads


def _released(ctx_field):
    if ctx_field is None:
        raise RuntimeError('Trying to backward through an engine pass a second time: its saved activations were released '
                           'by the first backward (retain_graph=True is not supported by engine.StackFn)')


WGRAD_BATCH = int(_os.environ.get('VLMO_WGRAD_BATCH', '2'))     # blocks per deferred weight-gradient launch; 0 = by tile count


def wgrad_batch_for(d, hid, cus=256, max_batch=4):
    """Blocks per batched weight-gradient launch.  Default: 2 (VLMo-Base: 108 output tiles of 256 x 256 per block -> 216 =
    one dispatch round).  VLMO_WGRAD_BATCH=0 picks the count whose tiles fill whole rounds (VLMo-Large: 192 per block -> 4
    blocks = 768 = exactly three rounds, where 2 blocks take two rounds for 1.5): measured, the side stream's rounds are not
    what the step waits for -- Large, 32 pairs, one box: (batch, temporary sets) = (2, 4) 24.80 ms, (4, 5) 25.35, (4, 6)
    24.91, (4, 8) 24.92, (2, 6) 24.85; Base (2, 4) 14.38, (4, 6) 14.48 -- the CUs a partial round leaves idle are taken by the
    main stream's kernels, and a batch of four holds its blocks' temporaries longer."""
    if WGRAD_BATCH > 0:
        return WGRAD_BATCH
    c = lambda n: -(-n // 256)
    tiles = c(d) * c(3 * d) + c(d) * c(d) + 2 * c(d) * c(hid)
    best, best_cost = 1, None
    for b in range(1, max_batch + 1):
        cost = -(-b * tiles // cus) / b
        if best_cost is None or cost < best_cost - 1e-9:
            best, best_cost = b, cost
    return best


TMP_SETS = 4                                                     # rotation depth of the backward temporaries
USE_STACK = True      # one StackFn call per pass; False (tests: no cross-block logic): one StackFn call per block

_PERSIST = {}


def _persist(dev, tag, numel, dtype):
    """Scratch that lives across passes (backward temporaries, column workspaces): keyed by the caller's stream,
    because reuse is ordered by that stream (vlmo_stack_bwd joins its side stream before it returns)."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream, tag)
    t = _PERSIST.get(key)
    if t is None or t.numel() < numel or t.dtype != dtype:
        t = _PERSIST[key] = torch.empty(numel, dtype=dtype, device=dev)
    return t


_EVENTS = {}


def _ready_events(dev, n):
    evs = _EVENTS.setdefault(dev, [])
    while len(evs) < n:
        evs.append(hip.event_create())
    return evs[:n]


INPLACE_ACCUM = _os.environ.get('VLMO_INPLACE_ACCUM', '1') != '0'      # kill switch for both mechanisms below

# ---- in-place gradient accumulation across the backward passes of one step -------------------------------------
# A four-objective step runs the block stack three to seven times; without a reducer every pass hands autograd a fresh
# gradient per parameter and the engine's input buffers add them: 337 elementwise launches = 1.4 ms of a 61 ms step.
#
# (1) WITHIN one backward() / autograd.grad() call, OPT-IN per call: `with engine.inplace_passes(loss): loss.backward()`.
#     The first StackFn node of the graph task that reaches a parameter GROUP (a block's shared parameters, or one
#     expert) returns views of a flat buffer and registers the buffer; every later node of the same task accumulates
#     INTO that buffer inside the weight-gradient kernels and returns None for the group.  That is only right while
#     autograd's input buffer for each parameter of the group still IS the first node's view when the later nodes have
#     run, i.e. while StackFn nodes are the parameter's only gradient producers: any other contribution (a weight
#     regulariser, a weight reused outside the engine) makes the input buffer add out of place -- the view shares its
#     storage with the flat buffer, so it cannot add in place -- and every later node would add into an orphaned
#     buffer, silently losing its gradient.  Whether that can happen is a property of the graph, so
#     inplace_passes() walks it from the roots before the backward (sole_producer_groups) and permits the mechanism only
#     for groups every trainable parameter of which is fed by StackFn nodes alone, and only to the nodes it walked,
#     during the first graph task that runs inside it.  Outside inplace_passes(), every pass returns fresh gradients and
#     autograd sums them.  Within those bounds .grad is never touched by us, which makes it correct under
#     autograd.grad(...) and backward(inputs=[...]) too.  Tensor hooks on a parameter see the sum: they run on the input
#     buffer when its AccumulateGrad node executes, after every producer.
# (2) ACROSS backward() calls (gradient-accumulation micro-steps, zero_grad(set_to_none=False)): a pass accumulates
#     straight into the views the parameters already hold as .grad.  AccumulateGrad adds any other contribution into
#     that .grad in place, so foreign producers are harmless here, but it is only right in an ordinary accumulating
#     backward(), so it is OPT-IN as well: `with engine.accumulate_into_grad():` around loss.backward().  The package's
#     NativeScalerWithGradNormCount (the reference loop's backward, utils.py:343-364) opts into both; bench.py into
#     neither.
_TASK_FLATS = {'task': None, 'flats': {}, 'nodes': None, 'groups': frozenset()}
_INTO_GRAD = [False]


class accumulate_into_grad:
    """Context manager: backward passes inside it may add into the gradient views parameters already hold."""

    def __init__(self, enabled=True):
        self.enabled = bool(enabled)

    def __enter__(self):
        self.prev = _INTO_GRAD[0]
        _INTO_GRAD[0] = self.enabled
        return self

    def __exit__(self, *a):
        _INTO_GRAD[0] = self.prev


def _walk(roots):
    """Every autograd node reachable from `roots` (tensors or nodes), and {id(parameter): (parameter, [the nodes that
    hand its AccumulateGrad node a gradient, one entry per edge])}."""
    stack = [r.grad_fn if isinstance(r, torch.Tensor) else r for r in roots]
    seen, feeds = set(), {}
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        for nxt, _ in fn.next_functions:
            if nxt is None:
                continue
            v = getattr(nxt, 'variable', None)
            if isinstance(v, torch.Tensor):
                feeds.setdefault(id(v), (v, []))[1].append(fn)
            stack.append(nxt)
    return seen, feeds


def sole_producer_groups(roots):
    """(engine nodes, {group key}): the StackFn nodes reachable from `roots`, and the parameter groups of theirs whose
    every trainable parameter receives its gradient from StackFn nodes ONLY and belongs to one group only -- the groups
    for which mechanism (1) is sound in a backward from exactly these roots.  An engine node is any node carrying
    `grad_groups` ([(group key, parameters)], set by StackFn.forward); every other op counts as a foreign producer."""
    seen, feeds = _walk(roots)
    nodes = [fn for fn in seen if getattr(fn, 'grad_groups', None) is not None]
    node_set = set(nodes)
    keys_of = {}                                     # id(parameter) -> group keys it belongs to
    for fn in nodes:
        for key, gp in fn.grad_groups:
            for p_ in gp:
                keys_of.setdefault(id(p_), set()).add(key)
    foreign = {pid for pid, (_, prod) in feeds.items() if any(fn not in node_set for fn in prod)}
    foreign |= {pid for pid, ks in keys_of.items() if len(ks) > 1}
    ok = set()
    bad = set()
    for fn in nodes:
        for key, gp in fn.grad_groups:
            if any(p_.requires_grad and id(p_) in foreign for p_ in gp):
                bad.add(key)
            else:
                ok.add(key)
    return node_set, frozenset(ok - bad)


class inplace_passes:
    """Context manager around ONE backward() / autograd.grad() from `roots` (the loss): lets the StackFn passes of that
    backward accumulate into one gradient buffer per parameter group (mechanism (1) above) wherever the graph shows
    that no other op produces a gradient for the group.  enabled=False (or INPLACE_ACCUM off): a no-op."""

    def __init__(self, *roots, enabled=True):
        self.roots = roots
        self.enabled = bool(enabled) and INPLACE_ACCUM

    def __enter__(self):
        self.prev = dict(_TASK_FLATS)       # (nested use restores the outer permit on exit)
        if self.enabled:
            nodes, groups = sole_producer_groups(self.roots)
            _TASK_FLATS.update(task=None, flats={}, nodes=nodes, groups=groups)
        else:
            _TASK_FLATS.update(nodes=None, groups=frozenset())
        return self

    def __exit__(self, *a):
        # the permit ends here, and the registry lets go of this backward's gradient buffers
        _TASK_FLATS.update(self.prev)


def _task_flats(node):
    """{group key: flat gradient buffer} of the running graph task, when an inplace_passes() walk permitted `node`;
    None otherwise.  The permit binds to the first graph task an engine node of it runs in."""
    if _TASK_FLATS['nodes'] is None or node not in _TASK_FLATS['nodes']:
        return None
    tid = torch._C._current_graph_task_id()
    if tid < 0:
        return None
    if _TASK_FLATS['task'] is None:
        _TASK_FLATS['task'] = tid
    elif _TASK_FLATS['task'] != tid:
        return None
    return _TASK_FLATS['flats']


def _group_key(gparams):
    # a weight matrix of the group (qkv weight / fc1 weight): gamma_1 may be a stand-in shared by all blocks (init_values=None)
    return gparams[QKV_W if len(gparams) == N_SHARED else FC1_W].data_ptr()


def _grad_flat(gparams, n):
    """The flat fp32 storage the group's parameters ALREADY hold as .grad in this engine's layout (views an earlier
    backward returned, possibly zeroed by zero_grad(set_to_none=False)), or None."""
    g = gparams[0].grad
    base = g._base if g is not None else None
    if base is None or g.dtype != torch.float32 or base.dim() != 1 or not base.is_contiguous():
        return None
    off = (g.data_ptr() - base.data_ptr()) // 4
    if off < 0 or off + n > base.numel():
        return None
    return base[off:off + n]


def _same_views(layout, flat):
    """Every parameter of the group holds as .grad exactly the view the layout carves out of `flat`, and nobody hooks it."""
    for p_, off in layout:
        if not p_.requires_grad:
            continue
        pg = p_.grad
        if pg is None or pg.data_ptr() != flat.data_ptr() + 4 * off or not pg.is_contiguous() or pg.dtype != torch.float32:
            return False
        if getattr(p_, '_post_accumulate_grad_hooks', None) or getattr(p_, '_backward_hooks', None):
            return False
    return True


# ---- the steps of StackFn.backward -------------------------------------------------------------------------------
_Scratch = namedtuple('_Scratch', 'nsets batch tb ws ws_n dxs')


def _backward_scratch(dev, nb, M, d, hid, B):
    """Scratch sizing: how many sets of backward temporaries rotate (nsets) and how many blocks share one deferred
    weight-gradient launch (batch), and the three persistent buffers: tb, the bf16 temporaries (TEMPS_BF16), one set
    per block in flight; ws, per set the column workspace of a block with up to 2 B attention sequences (ws_n fp32
    each, laid out by vlmo_stack_bwd_ws_bytes); dxs, the dx ping-pong and dx1."""
    want = wgrad_batch_for(d, hid)
    nsets = max(1, min(max(TMP_SETS, want + 1), nb))
    batch = max(1, min(want, nsets - 1)) if nb > nsets else max(1, want)
    tb = _persist(dev, 'tb', nsets * _layouts(d, hid).temps.cols * M, torch.bfloat16)
    ws_n = hip.lib().vlmo_stack_bwd_ws_bytes(M, d, hid, 2 * B) // 4
    ws = _persist(dev, 'ws', nsets * ws_n, torch.float32)
    dxs = _persist(dev, 'dx', 3 * M * d, torch.float32)
    return _Scratch(nsets, batch, tb, ws, ws_n, dxs)


def _sink_buckets(sink, groups, d, hid, dev):
    """Sink route: the buckets of one block from the gradient reducer, [(flat, fresh)] per group.  The groups of a block
    sit next to each other in one arena (named by the block's first parameter, with room for every expert the block
    owns) so that the reducer sends them as one collective; fresh = nothing fed the bucket yet in this window."""
    akey = id(groups[0].params[0])
    aroom = group_numel(groups[0], d, hid) + ARENA_EXPERTS * group_numel(groups[1], d, hid)
    return [sink.acquire(g.params, group_numel(g, d, hid), dev, akey, aroom, layout=group_layout(g, d, hid), lazy_zero=True)
            for g in groups]


FRESH, FROM_TASK, FROM_GRAD = 0, 1, 2       # where _local_bucket found a group's bucket


def _local_bucket(g, d, hid, wanted, reg, permitted, into_grad, fresh):
    """Local route (no reducer): the gradient bucket of ONE group and how it was obtained.
    wanted: the graph task asks for the gradient of every trainable parameter of the group -- accumulating in place is
    only considered then.  reg: the running task's {group key: flat} when an inplace_passes() walk permitted this node,
    else None; permitted: the group keys that walk found to have no other producer; into_grad: inside
    accumulate_into_grad(); fresh(): new storage for the bucket.
      FROM_TASK  an earlier node of this graph task registered a buffer for the group: accumulate into it;
      FROM_GRAD  the parameters hold exactly this layout's views of one flat buffer as .grad, unhooked (an earlier
                 backward of the step): accumulate into that;
      FRESH      new storage, handed to autograd -- and registered for the later nodes of the task only when the walk
                 permitted the group."""
    key = _group_key(g.params)
    if wanted:
        if reg is not None and key in reg:
            return reg[key], FROM_TASK
        if into_grad:
            have = _grad_flat(g.params, group_numel(g, d, hid))
            if have is not None and _same_views(group_layout(g, d, hid), have):
                return have, FROM_GRAD
    flat = fresh()
    if wanted and reg is not None and key in permitted:
        reg[key] = flat
    return flat, FRESH


def _local_buckets(groups, wants, d, hid, reg, permitted, into_grad, storage, off):
    """Local route for one block: [(flat, fresh)] per group like _sink_buckets, and the storage offset behind the block.
    wants: needs_input_grad of the block's parameters; storage(off, n): fresh storage (every group has its place in
    it, taken or not)."""
    got = []
    for g in groups:
        n = group_numel(g, d, hid)
        wanted = all(w or not p_.requires_grad for p_, w in zip(g.params, wants[g.lo:g.hi]))
        flat, how = _local_bucket(g, d, hid, wanted, reg, permitted, into_grad, lambda: storage(off, n))
        got.append((flat, how == FRESH))
        off += n
    return got, off


def _fresh_storage(numel, dev):
    """storage(off, n) -> [off, off + n) of ONE fp32 buffer of `numel` elements, allocated when first asked for."""
    whole = []

    def storage(off, n):
        if not whole:
            whole.append(torch.empty(numel, dtype=torch.float32, device=dev))
        return whole[0][off:off + n]
    return storage


def _wire_temporaries(D, k, nb, M, d, hid, sc, dxo, dx_in):
    """Temporaries of the k-th block the backward processes: its set of the rotating bf16 temporaries and workspaces,
    and the dx chain (dx2 = incoming: dxo for the first, else the previous block's dx0; dx0 = outgoing: dx_in for the
    last, else the other half of the ping-pong)."""
    st_, md, T = k % sc.nsets, M * d, _layouts(d, hid).temps
    T.wire(D, sc.tb.data_ptr() + st_ * T.cols * M * 2, M, 2)
    D.ws_main, D.ws_bytes = sc.ws.data_ptr() + st_ * sc.ws_n * 4, sc.ws_n * 4
    D.dx1 = sc.dxs.data_ptr() + 2 * md * 4
    D.dx2 = dxo.data_ptr() if k == 0 else sc.dxs.data_ptr() + ((k - 1) % 2) * md * 4
    D.dx0 = dx_in.data_ptr() if k == nb - 1 else sc.dxs.data_ptr() + (k % 2) * md * 4


def _zero_buckets(acquired, store_ok, d, hid):
    """Zeroing.  acquired: (flat, fresh, is_expert) of every bucket of the pass.  In store mode (every bucket fresh) the
    deferred launches WRITE the weight-gradient matrices, so only the vector gradients (accumulated with atomics by the
    column folds) are zeroed, in one multi-tensor fill: the vector runs of SHARED_GRADS / EXPERT_GRADS (two per
    bucket).  Otherwise the launches accumulate, and the fresh buckets are zeroed whole."""
    if store_ok:
        buckets = _layouts(d, hid).buckets
        torch._foreach_zero_([f_[lo:hi] for f_, _, is_exp in acquired for lo, hi in buckets[is_exp].vectors])
    else:
        for f_, fr, _ in acquired:
            if fr:
                f_.zero_()


def _hand_to_sink(sink, groups, spans, grads_all, evs):
    """Hand-off under a reducer, block by block in backward order: the parameters take their bucket views as .grad
    (autograd is handed nothing), then the block's buckets are released behind its grad_ready event."""
    for i in reversed(range(len(groups))):
        o = spans[i][0]
        for g in groups[i]:
            for p_, g_ in zip(g.params, grads_all[o + g.lo:o + g.hi]):
                if p_.requires_grad:
                    if p_.grad is None:
                        p_.grad = g_
                    elif p_.grad.data_ptr() != g_.data_ptr():
                        raise RuntimeError('a parameter of a data-parallel block already holds a foreign .grad; '
                                           'use zero_grad(set_to_none=True)')
        sink.release_all([g.params for g in groups[i]], ready_event=evs[i] if evs is not None else None)


def _run_captures(metas, SB, sc, M, d, hid):
    """BlockMeta.capture of the blocks that asked for one, after vlmo_stack_bwd: views (no copy) of the block's saved qkv
    rows in the forward slab SB and of its dctx in the rotating temporaries.  Nothing in a block's backward writes
    dy2 = dctx after the attention backward has read it (block.hip: the fc2 backward writes dy2, the LayerNorm backward
    reads it, the proj backward overwrites it with dctx), so the set of the k-th processed block holds its dctx until
    block k + nsets takes the set: a captured block must be among the last nsets processed -- a one-block StackFn always
    is, which is how VLMO.attention_gradcam runs the layers it is asked for."""
    nb, L = len(metas), _layouts(d, hid)
    for k in range(nb):
        i = nb - 1 - k
        if metas[i].capture is None:
            continue
        if k + sc.nsets < nb:
            raise RuntimeError(f'the backward temporaries of block {i} of this {nb}-block stack were reused before its '
                               f'capture could run ({sc.nsets} sets rotate): run a captured block as a one-block StackFn')
        qkv, dctx = L.slab.view(SB, i, M, 'qkv'), L.temps.view(sc.tb, k % sc.nsets, M, 'dctx')
        metas[i].capture(qkv, dctx, metas[i].plan, metas[i].fused)


class StackFn(torch.autograd.Function):
    """All Blocks of one backbone pass (the loops at vlmo.py:402-411) as ONE native call per direction
    (vlmo_stack_fwd / vlmo_stack_bwd).  metas: one BlockMeta per block, in forward order; params: the blocks'
    parameter lists concatenated, each in per-block order (vlmo.Block._params)."""

    @staticmethod
    def forward(ctx, x, metas, *params):
        nb = len(metas)
        m0 = metas[0]
        pl, d, H, hid = m0.plan, m0.d, m0.heads, m0.hidden
        M, dev = x.shape[0], x.device
        need_bwd = any(ctx.needs_input_grad)
        x = x.contiguous()
        # every buffer of the layouts starts 128-byte aligned then (the GEMMs need K % 64 == 0 anyway)
        assert d % 64 == 0 and hid % 64 == 0, (d, hid)
        spans, groups, pofs = [], [], 0     # per block: (offset, count) in params, and its parameter groups
        for mt in metas:
            npar = N_SHARED + N_EXPERT * len(mt.expert_ranges)
            spans.append((pofs, npar))
            groups.append(block_groups(params[pofs:pofs + npar]))
            pofs += npar
        # per block: one bf16 slab (SLAB_BF16) and one fp32 slab (SLAB_F32, then the log-sum-exp rows); the blocks'
        # outputs x2 (= the next block's saved input)
        L = _layouts(d, hid)
        launches = [pl.attn_launches(mt.fused) for mt in metas]
        sb_n = L.slab.cols * M
        sf_n = [L.f32.cols * M + sum(n for _, n in _lse_layout(ln, H)) for ln in launches]
        live = nb if need_bwd else 1        # without a backward every block reuses the first block's slabs
        SB = torch.empty(live * sb_n, dtype=torch.bfloat16, device=dev)
        SF = torch.empty(sum(sf_n[:live]) if need_bwd else max(sf_n), dtype=torch.float32, device=dev)
        X2 = torch.empty((nb if need_bwd else min(nb, 2), M, d), dtype=torch.float32, device=dev)
        descs = (hip.BlockDesc * nb)()
        keep = [SB, SF, X2, pl]
        if m0.shadows is not None:          # every stale weight shadow of the pass in one launch (ShadowCache.refresh)
            stale = []
            for (sh, *ex) in groups:
                stale += [sh.params[QKV_W], sh.params[PROJ_W]] + [g.params[FC1_W] for g in ex] + [g.params[FC2_W] for g in ex]
            m0.shadows.refresh(stale)
        sf_off = 0
        xin = x.data_ptr()
        for i, mt in enumerate(metas):
            D = descs[i]
            pb = SB.data_ptr() + (i * sb_n * 2 if need_bwd else 0)
            pf = SF.data_ptr() + (sf_off * 4 if need_bwd else 0)
            sf_off += sf_n[i]
            x2 = X2[i if need_bwd else i % 2]
            _fill_forward(D, mt, groups[i], launches[i], M, pb, pf, need_bwd, keep)
            D.x, D.x2 = xin, x2.data_ptr()
            xin = x2.data_ptr()
        S = hip.StackDesc()
        S.n_blocks = nb
        S.blocks = ctypes.cast(descs, ctypes.POINTER(hip.BlockDesc))
        hip.stack_fwd(S)
        out = X2[(nb - 1) if need_bwd else (nb - 1) % 2]
        if need_bwd:
            ctx.metas, ctx.descs, ctx.keep, ctx.spans, ctx.groups = metas, descs, keep, spans, groups
            ctx.save_for_backward(x, *params)
            ctx.sink = GRAD_SINK
            if ctx.sink is None:
                # the parameter groups this node produces gradients for, read by inplace_passes()' graph walk
                ctx.grad_groups = [(_group_key(g.params), g.params) for blk in groups for g in blk]
            else:
                # ... and, per block, by the reducer's (dp.GradReducer.prepare), which counts one backward call per group
                ctx.sink_groups = [[g.params for g in blk] for blk in groups]
                for blk in ctx.sink_groups:
                    for gp in blk:
                        ctx.sink.expect(gp)
        return out

    @staticmethod
    def backward(ctx, dxo):
        metas, descs, spans, groups = ctx.metas, ctx.descs, ctx.spans, ctx.groups
        _released(descs)
        x, *params = ctx.saved_tensors
        nb = len(metas)
        m0 = metas[0]
        d, hid = m0.d, m0.hidden
        M, dev = x.shape[0], x.device
        dxo = dxo.contiguous()
        sink = ctx.sink
        sc = _backward_scratch(dev, nb, M, d, hid, m0.plan.B)
        dx_in = torch.empty((M, d), dtype=torch.float32, device=dev)
        if sink is None:
            storage = _fresh_storage(sum(group_numel(g, d, hid) for blk in groups for g in blk), dev)
            reg = _task_flats(ctx) if INPLACE_ACCUM else None
            permitted, into_grad, off = _TASK_FLATS['groups'], INPLACE_ACCUM and _INTO_GRAD[0], 0
        grads_all = [None] * len(params)
        store_ok, acquired = True, []       # (flat, fresh, is_expert) of every gradient bucket of the pass
        for k in range(nb):                 # backward order: k-th processed block is i = nb-1-k
            i = nb - 1 - k
            D, blk, (o, n_) = descs[i], groups[i], spans[i]
            if sink is not None:
                got = _sink_buckets(sink, blk, d, hid, dev)
            else:
                got, off = _local_buckets(blk, ctx.needs_input_grad[2 + o:2 + o + n_], d, hid, reg, permitted, into_grad,
                                          storage, off)
            # a bucket that an earlier pass of the step already fed is accumulated into: no store mode for this pass
            store_ok = store_ok and all(fr for _, fr in got)
            acquired += [(f_, fr, g.lo > 0) for g, (f_, fr) in zip(blk, got)]
            grads = _fill_grads(D, [f_ for f_, _ in got], d, hid, len(blk) - 1)
            for g, (_, fr) in zip(blk, got):
                if fr or sink is not None:  # groups accumulated in place hand nothing to autograd
                    grads_all[o + g.lo:o + g.hi] = grads[g.lo:g.hi]
            _split_backward_attention(D, metas[i])
            _wire_temporaries(D, k, nb, M, d, hid, sc, dxo, dx_in)
        _zero_buckets(acquired, store_ok, d, hid)
        S = hip.StackDesc()
        S.n_blocks, S.wgrad_batch, S.n_tmp_sets, S.wgrad_store = nb, sc.batch, sc.nsets, int(store_ok)
        S.blocks = ctypes.cast(descs, ctypes.POINTER(hip.BlockDesc))
        side = _side_stream(dev) if _use_side_stream(sink, M) else None
        S.side_stream = side.cuda_stream if side is not None else None
        evs = None
        if sink is not None and side is not None:
            evs = _ready_events(dev, nb)
            arr = (ctypes.c_void_p * nb)(*evs)
            S.grad_ready = ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))
        hip.stack_bwd(S)
        if any(mt.capture is not None for mt in metas):
            _run_captures(metas, ctx.keep[0], sc, M, d, hid)
        ctx.descs = ctx.keep = None
        if sink is not None:
            _hand_to_sink(sink, groups, spans, grads_all, evs)
            return (dx_in, None) + (None,) * len(params)
        return (dx_in, None, *grads_all)


class FinalNormFn(torch.autograd.Function):
    """self.norm (vlmo.py:413) writing the [B, T+P, d] fp32 output through the row map."""

    @staticmethod
    def forward(ctx, x, w, b, plan, out_shape, eps=LN_EPS):
        M, d = x.shape
        # a plan with text lengths leaves the rows of the dropped positions unwritten: they are exactly 0
        full = M == plan.B * (plan.T + plan.P)
        out = (torch.empty if full else torch.zeros)(out_shape, dtype=torch.float32, device=x.device)
        mean, rstd = torch.empty(M, device=x.device), torch.empty(M, device=x.device)
        hip.ln_fwd(x, w, b, out, mean, rstd, plan.rowmap, M, d, eps)
        ctx.plan = plan
        ctx.save_for_backward(x, w, mean, rstd)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w, mean, rstd = ctx.saved_tensors
        M, d = x.shape
        dout = dout.contiguous().float()
        dx = torch.empty_like(x)
        dw, db = torch.zeros_like(w), torch.zeros_like(w)
        hip.ln_bwd(dout, ctx.plan.rowmap, x, w, mean, rstd, None, dx, dw, db, M, d)
        return dx, dw, db, None, None, None


class EmbedFn(torch.autograd.Function):
    """embed_txt + embed_img (vlmo.py:298-324) into one packed fp32 [M, d] matrix.

    tensor args: patch_w [d,C,p,p], patch_b, cls_tok, mask_tok, pos_embed [1,P,d], type_emb [2or3,d],
                 word, tpos, btype, ln_w, ln_b   (any of the two groups may be unused)"""

    @staticmethod
    def forward(ctx, meta, patch_w, patch_b, cls_tok, mask_tok, pos_embed, type_emb, word, tpos, btype,
                ln_w, ln_b):
        pl, d, dev = meta['plan'], meta['d'], meta['device']
        img, ids, masked = meta['img'], meta['ids'], meta['masked']
        B, T, P = pl.B, pl.T, pl.P
        x = torch.empty((pl.M, d), dtype=torch.float32, device=dev)
        drop, seed, sh = meta['drop'], meta['seed'], meta['shadows']
        saved = {}
        if T:
            xhat = torch.empty((pl.nt, d), dtype=torch.float32, device=dev)
            rstd = torch.empty((pl.nt,), dtype=torch.float32, device=dev)
            if pl.txt_lens is None:
                hip.embed_txt_fwd(ids, word, tpos, btype[0], ln_w, ln_b, type_emb[0], x[:pl.nt], xhat, rstd, B, T, d,
                                  meta['txt_eps'], drop=drop, seed=seed + 1)
            else:
                hip.embed_txt_rows_fwd(ids, pl.txt_src, word, tpos, btype[0], ln_w, ln_b, type_emb[0], x[:pl.nt], xhat,
                                       rstd, pl.nt, T, d, meta['txt_eps'], drop=drop, seed=seed + 1)
            saved['txt'] = (xhat, rstd)
        if P:
            npatch = P - 1
            p = meta['patch']
            patches = torch.empty((B * npatch, patch_w[0].numel()), dtype=torch.bfloat16, device=dev)
            hip.patchify(img, patches, p)
            proj = torch.empty((B * npatch, d), dtype=torch.bfloat16, device=dev)
            K = patches.shape[1]
            hip.gemm_nt(hip.EPI_BIAS, patches, sh.get(patch_w, need_t=False)[0], B * npatch, d, K, proj,
                        bias=patch_b)
            hip.embed_img_finish(proj, cls_tok, mask_tok, pos_embed, type_emb[meta['img_type']], masked,
                                 x[pl.nt:], B, npatch, d, drop=drop, seed=seed + 2)
            saved['img'] = patches
        ctx.meta, ctx.saved = meta, saved
        ctx.save_for_backward(patch_w, type_emb, word, ln_w)
        return x

    @staticmethod
    def backward(ctx, dx):
        meta, saved = ctx.meta, ctx.saved
        patch_w, type_emb, word, ln_w = ctx.saved_tensors
        pl, d, dev = meta['plan'], meta['d'], meta['device']
        B, T, P = pl.B, pl.T, pl.P
        drop, seed = meta['drop'], meta['seed']
        dx = dx.contiguous()
        g = [None] * 11   # patch_w, patch_b, cls, mask, pos, type, word, tpos, btype, ln_w, ln_b
        # every parameter gradient of the embeddings is a view of ONE zero-filled buffer (one fill launch instead of eleven)
        npatch = P - 1 if P else 0
        shapes = [tuple(type_emb.shape)]
        if T:
            shapes += [tuple(word.shape), (meta['tpos_rows'], d), (2, d), (d,), (d,)]
        if P:
            shapes += [(d,), (d,), (P, d), (d, saved['img'].shape[1]), (d,)]
        sizes = [int(torch.Size(sh).numel()) for sh in shapes]
        flat = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
        views, o = [], 0
        for sh, n in zip(shapes, sizes):
            views.append(flat[o:o + n].view(sh))
            o += n
        dtype_emb = views[0]
        k = 1
        if T:
            xhat, rstd = saved['txt']
            dword, dtpos_full, dbtype, dlnw, dlnb = views[k:k + 5]
            k += 5
            if pl.txt_lens is None:
                hip.embed_txt_bwd(dx[:pl.nt], meta['ids'], xhat, rstd, ln_w, dword, dtpos_full[:T], dbtype[0], dlnw, dlnb,
                                  dtype_emb[0], B, T, d, drop=drop, seed=seed + 1)
            else:
                hip.embed_txt_rows_bwd(dx[:pl.nt], meta['ids'], pl.txt_off, xhat, rstd, ln_w, dword, dtpos_full[:T],
                                       dbtype[0], dlnw, dlnb, dtype_emb[0], B, T, pl.maxT, d, drop=drop, seed=seed + 1)
            g[6], g[7], g[8], g[9], g[10] = dword, dtpos_full, dbtype, dlnw, dlnb
        if P:
            patches = saved['img']
            dproj = torch.empty((B * npatch, d), dtype=torch.bfloat16, device=dev)
            dcls, dmask, dpos, dpw, dpb = views[k:k + 5]
            hip.embed_img_bwd(dx[pl.nt:], meta['masked'], dproj, dcls, dmask, dpos, dtype_emb[meta['img_type']],
                              B, npatch, d, drop=drop, seed=seed + 2)
            hip.gemm_tn(dproj, patches, dpw, B * npatch, d, patches.shape[1])
            hip.colsum(dproj, dpb, B * npatch, d)
            g[0], g[1] = dpw.view_as(patch_w), dpb
            g[2], g[4] = dcls, dpos
            g[3] = dmask if meta['masked'] is not None else None
        g[5] = dtype_emb
        return (None, *g)
