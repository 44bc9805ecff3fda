"""TEST INFRASTRUCTURE ONLY: a deterministic harness around the real ``zero.ZeroAdam`` -- no model, no autograd, no process
group.  One process plays rank ``r`` of ``W``: the buckets are the real ``dp._Bucket`` / ``dp._SinkBucket`` filled by hand
(``shard32`` = the rank's slice of a full flat gradient, ``had`` per parameter), the reducer is a stub whose
``all_reduce_now`` adds the squared norm of everybody else's gradient, and the reference is ``oracle.adamw_oracle`` in fp64
on the WHOLE tensors with the WHOLE gradient (it does not know about ranks, slices or chunks); the rank's result is compared
on its slice, and everything the rank must not touch is compared bit for bit.

tests/test_zero_slices_cpu.py runs it on ``EmuZero`` (the two kernel calls restated in torch over the launch table),
tests/test_zero_slices_gpu.py on ``CheckedZero`` (the HIP kernels).

Bounds (all from tests/test_optim_gpu.py, which states them for the same kernels on whole tensors):
  norm, clip coefficient   1e-5 relative                                  (test_fused_clip_matches_clip_grad_norm)
  parameters               S * (2e-6 max|p_ref| + 1e-7) after S steps     (per-step fp32 round-off of the update)
  moments                  rtol 1e-5, atol 1e-8 (m), 1e-10 (v)
"""
import functools

import numpy as np
import torch

from exploremultimodal_amd import dp, mt
from exploremultimodal_amd.zero import ZeroAdam
from oracle import adamw_oracle

BETAS, EPS = (0.9, 0.98), 1e-8
GROUPS = [(2e-3, 0.05), (5e-4, 0.0), (1e-3, 0.1)]          # (lr, weight decay); parameter i of a bucket is in group i % 3
# hook bucket: starts 0, 1, 6, 39, 65578, 66578, 66582 -> 0, 4, 8 and 12 bytes off 16-byte alignment; parameter 3 is
# misaligned and longer than mt.CHUNK, parameter 0 has one element
HOOK_SHAPES = [(1,), (5,), (33,), (65536 + 3,), (40, 25), (4,), (70001,)]
HOOK_NEVER = 4          # had == False in every step (its gradient range holds garbage that must not be read)
HOOK_LATE = 2           # has no gradient in the second step: its counter falls behind, two launches in the third
# sink bucket: holes in the layout (the qkv bias hole of the engine's buckets) and padding at the end
SINK_SHAPES = [(6,), (35,), (3, 43), (3,)]
SINK_GAPS = [7, 0, 3]
STEPS = 3
WORLDS = (1, 2, 3, 8)
GARBAGE = 3.0           # what gradient ranges outside every stepping entry hold
# beside the main case (AdamW, clip 1.0 below the norm, every W): keyword arguments of Sim, run at W = 3
VARIANTS = {
    'no_clip': dict(clip=None),
    'l2_mode': dict(adam_w=False),
    'inf_in_own_slice': dict(bad_step=1, bad_where='own'),
    'inf_in_other_ranks': dict(bad_step=1, bad_where='other'),
}


def _numel(shape):
    return int(np.prod(shape))


def sink_layout_offsets():
    offs, n = [], 0
    for i, s in enumerate(SINK_SHAPES):
        offs.append(n)
        n += _numel(s) + (SINK_GAPS[i] if i < len(SINK_GAPS) else 0)
    return offs, n


def hook_offsets():
    offs, n = [], 0
    for s in HOOK_SHAPES:
        offs.append(n)
        n += _numel(s)
    return offs, n


def had_at(step):
    return [not (i == HOOK_NEVER or (i == HOOK_LATE and step == 1)) for i in range(len(HOOK_SHAPES))]


# ---------------------------------------------------------------------------------------------- inputs and the oracle
@functools.lru_cache(maxsize=None)
def initial_params():
    """fp32 initial values, per bucket ('sink', 'hook') a tuple of 1-D arrays (read-only)."""
    g = torch.Generator().manual_seed(0)
    out = {}
    for name, shapes in (('sink', SINK_SHAPES), ('hook', HOOK_SHAPES)):
        out[name] = tuple((torch.randn(_numel(s), generator=g) * 0.5).numpy() for s in shapes)
        for a in out[name]:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gradients(step):
    """The full flat fp32 gradient of each bucket (its unpadded length; holes hold GARBAGE), read-only."""
    g = torch.Generator().manual_seed(1000 + step)
    out = {}
    for name, (offs, n), shapes in (('sink', sink_layout_offsets(), SINK_SHAPES), ('hook', hook_offsets(), HOOK_SHAPES)):
        flat = np.full(n, GARBAGE, np.float32)
        for off, s in zip(offs, shapes):
            flat[off:off + _numel(s)] = (torch.randn(_numel(s), generator=g) * (0.1 * (step + 1))).numpy()
        flat.setflags(write=False)
        out[name] = flat
    return out


def stepping(name, step):
    """[(index, offset, numel)] of the bucket's parameters that step in `step`."""
    if name == 'sink':
        offs, _ = sink_layout_offsets()
        return [(i, off, _numel(s)) for i, (off, s) in enumerate(zip(offs, SINK_SHAPES))]
    offs, _ = hook_offsets()
    had = had_at(step)
    return [(i, off, _numel(s)) for i, (off, s) in enumerate(zip(offs, HOOK_SHAPES)) if had[i]]


@functools.lru_cache(maxsize=None)
def oracle_run(adam_w, clip, bad_step):
    """The fp64 trajectory on whole tensors: per step a dict with 'norm', 'coef', 'bad' and per bucket the lists 'p', 'm',
    'v' (one fp64 array per parameter) AFTER the step.  Computed once per variant and shared by every rank of every world
    size.  ``bad_step``: the step whose gradient is not finite -- nothing moves, and the step still counts for the bias
    corrections of the parameters that would have stepped (optim.FusedAdam counts such steps, and torch.optim.AdamW under
    GradScaler does not: this project follows its own FusedAdam, test_zero_slices_gpu.py pins the two to each other)."""
    init = initial_params()
    st = {name: {'p': [a.astype(np.float64) for a in init[name]], 'm': [np.zeros(a.size) for a in init[name]],
                 'v': [np.zeros(a.size) for a in init[name]], 'n': [0] * len(init[name])} for name in ('sink', 'hook')}
    out = []
    for step in range(STEPS):
        gr = gradients(step)
        parts = [gr[name][off:off + n] for name in ('sink', 'hook') for _, off, n in stepping(name, step)]
        norm, coef = adamw_oracle.clip_coef(parts, clip)
        bad = step == bad_step
        for name in ('sink', 'hook'):
            s = st[name]
            for i, off, n in stepping(name, step):
                s['n'][i] += 1
                if bad:
                    continue
                lr, wd = GROUPS[i % len(GROUPS)]
                s['p'][i], s['m'][i], s['v'][i] = adamw_oracle.adam_step(
                    s['p'][i], gr[name][off:off + n].astype(np.float64) * coef, s['m'][i], s['v'][i], s['n'][i], lr,
                    BETAS[0], BETAS[1], EPS, wd, adam_w_mode=adam_w)
        out.append({'norm': norm, 'coef': coef, 'bad': bad,
                    **{name: {k: [a.copy() for a in st[name][k]] for k in 'pmv'} for name in ('sink', 'hook')}})
    return out


# ---------------------------------------------------------------------------------------------- the optimizers under test
class Broke(AssertionError):
    """A check of the harness failed.  ``kinds``: which -- 'table' (a launch table points outside the optimizer's buffers or
    does not cover its entries), 'norm' (norm or clip coefficient), 'untouched' (something outside the stepping entries
    changed), 'value' (a parameter or a moment of the slice is off the oracle).  The harness's own set-up uses plain
    asserts, so a broken harness is not mistaken for a caught error."""

    def __init__(self, kinds, info):
        super().__init__(f'{sorted(kinds)}: {info}')
        self.kinds = set(kinds)


def _table(cond, *info):
    if not cond:
        raise Broke({'table'}, info)


class CheckedZero(ZeroAdam):
    """ZeroAdam with the HIP kernels, whose launch tables are walked first: every chunk of every column must lie inside
    this optimizer's own buffer of that kind (flat parameters, gradient shards, first and second moments) before a kernel
    gets the addresses."""
    check_cover = True      # test_zero_slices_cpu.py turns this one check off to show that the value checks see the same error

    def _spans(self):
        out = []
        for pt in self.parts:
            for kind, t in zip('pmvg', (pt.pflat, pt.m, pt.v, pt.bucket.shard32)):
                if t is not None:
                    out.append((kind, t.data_ptr(), t.data_ptr() + 4 * t.numel(), t))
        return out

    def walk(self, tab):
        """[(tensor index, p, g, m, v)] per chunk: slices of the owning buffers, found from the DEVICE tables the kernels
        read (``tab.dev_i``, ``tab.dev_c``) and the struct's own pointers, not from ``tab.ent``."""
        nt, tl = tab.nt, tab.tl
        base = tab.dev_i.data_ptr()
        _table([tl.p, tl.g, tl.m, tl.v, tl.numel, tl.chunk_start] == [base + 8 * nt * k for k in range(6)] or nt == 0, 'struct')
        _table(tl.chunk_tensor == tab.dev_c.data_ptr() or tab.n_chunks == 0, 'struct')
        _table(tl.chunk == mt.CHUNK and tl.n_chunks == tab.n_chunks == tab.dev_c.numel(), 'chunk count')
        _table(tab.dev_i.numel() == 5 * nt + tab.n_chunks, 'table size')
        if nt:
            _table((tl.lr, tl.wd) == (tab.dev_f.data_ptr(), tab.dev_f.data_ptr() + 4 * nt), 'lr / wd')
        ti, ct = tab.dev_i.cpu().tolist(), tab.dev_c.cpu().tolist()
        cols, numel, cs = [ti[k * nt:(k + 1) * nt] for k in range(4)], ti[4 * nt:5 * nt], ti[5 * nt:]
        spans = self._spans()
        out, covered = [], [0] * nt
        for t, off in zip(ct, cs):
            _table(0 <= t < nt and 0 <= off < numel[t], 'chunk outside its tensor', t, off)
            n = min(tl.chunk, numel[t] - off)
            views = []
            for kind, col in zip('pgmv', cols):
                a = col[t] + 4 * off
                own = [(lo, buf) for k, lo, hi, buf in spans if k == kind and lo <= a and a + 4 * n <= hi]
                _table(own, f'entry {t}: {kind} range [{a:#x}, +{4 * n}) lies outside every {kind} buffer of the optimizer')
                lo, buf = own[0]
                views.append(buf[(a - lo) // 4:(a - lo) // 4 + n])
            covered[t] += n
            out.append((t, *views))
        if self.check_cover:
            _table(covered == numel, 'the chunks do not cover every tensor exactly once')
        return out

    def _local_sqnorm(self, tab):
        self.walk(tab)
        return super()._local_sqnorm(tab)

    def _apply(self, tab, args, ctl):
        self.walk(tab)
        super()._apply(tab, args, ctl)


class EmuZero(CheckedZero):
    """The two kernel calls (``vlmo_mt_grad_norm``, ``vlmo_mt_adam``) restated in fp32 torch over the launch table, chunk by
    chunk, for the machines without a GPU."""

    def _local_sqnorm(self, tab):
        partial = [float((g * g).sum(dtype=torch.float64).float()) for _, _, g, _, _ in self.walk(tab)]
        norm = torch.tensor(sum(partial), dtype=torch.float64).float().sqrt()      # inv_scale 1, max_norm 0
        bad = not bool(torch.isfinite(norm)) or float(norm) > 3.0e38
        tab.ctl[0], tab.ctl[1], tab.ctl[2] = norm, 0.0 if bad else 1.0, 1.0 if bad else 0.0
        return tab.ctl[0] * tab.ctl[0]

    def _apply(self, tab, a, ctl):
        if ctl is not None and float(ctl[2]) != 0:
            return
        gs = ctl[1].clone() if ctl is not None else torch.tensor(1.0)
        nt = tab.nt
        for t, p, g, m, v in self.walk(tab):
            lr, wd = tab.dev_f[t].clone(), tab.dev_f[nt + t].clone()
            g = g * gs
            if not a.adam_w_mode:
                g = g + wd * p
            m.mul_(a.beta1).add_(g * (1.0 - a.beta1))
            v.mul_(a.beta2).add_(g * g * (1.0 - a.beta2))
            u = (m * a.inv_bc1) / ((v * a.inv_bc2).sqrt() + a.eps)
            if a.adam_w_mode:
                u = u + wd * p
            p.sub_(lr * u)


# ---------------------------------------------------------------------------------------------- one simulated rank
class StubReducer:
    """What ZeroAdam asks of a ``dp.GradReducer``, without a process group."""
    reduce_scatter = True

    def __init__(self, world, rank, device):
        self.world, self.rank, self.device = world, rank, torch.device(device)
        self.sinks, self.buckets, self._sink_params = {}, [], set()
        self.other_sq = 0.0         # sum of squares of the stepping gradient outside this rank's slices (fp64)
        self.reduces, self.gathers = 0, []

    def all_reduce_now(self, t):
        t += self.other_sq
        self.reduces += 1

    def all_gather(self, out, src):
        self.gathers.append((out, src))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


class Sim:
    """Rank `rank` of `world` with fresh parameters.  ``run()`` takes the STEPS steps and asserts after each; the worst
    error / bound ratios it saw are left in ``self.worst``."""

    def __init__(self, world, rank, device, cls=EmuZero, adam_w=True, clip=1.0, bad_step=None, bad_where='own'):
        self.world, self.rank, self.device = world, rank, torch.device(device)
        self.adam_w, self.clip, self.bad_step, self.bad_where = adam_w, clip, bad_step, bad_where
        init = initial_params()
        mk = lambda a, s: torch.nn.Parameter(torch.from_numpy(a.copy()).reshape(s).to(self.device))
        self.params = {'sink': [mk(a, s) for a, s in zip(init['sink'], SINK_SHAPES)],
                       'hook': [mk(a, s) for a, s in zip(init['hook'], HOOK_SHAPES)]}
        red = self.red = StubReducer(world, rank, self.device)
        offs, n = sink_layout_offsets()
        sb = dp._SinkBucket(n, self.device, torch.float32, world, params=tuple(self.params['sink']),
                            layout=list(zip(self.params['sink'], offs)))
        hb = dp._Bucket('hook', self.params['hook'], self.device, torch.float32, world)
        assert hb.offsets == hook_offsets()[0]
        for b in (sb, hb):
            assert b.padded > b.numel and b.padded % world == 0         # there is padding at the end
            b.shard32 = torch.zeros(b.padded // world, dtype=torch.float32, device=self.device)
            b.has_grad = True
        red.sinks['block'] = sb
        red.buckets.append(hb)
        red._sink_params.update(id(p) for p in self.params['sink'])
        self.buckets = {'sink': sb, 'hook': hb}
        groups = [{'params': [], 'lr': lr, 'weight_decay': wd} for lr, wd in GROUPS]
        for name in ('sink', 'hook'):
            for i, p in enumerate(self.params[name]):
                groups[i % len(GROUPS)]['params'].append(p)
        self.opt = cls(red, groups, betas=BETAS, eps=EPS, adam_w_mode=adam_w)
        self.worst = {}

    def _note(self, what, ratio):
        self.worst[what] = max(self.worst.get(what, 0.0), float(ratio))

    def _own_mask(self, name, step):
        """bool over the padded bucket: elements of stepping parameters inside this rank's slice; and the slice."""
        b = self.buckets[name]
        n = b.padded // self.world
        lo, hi = self.rank * n, (self.rank + 1) * n
        stepmask = np.zeros(b.padded, bool)
        for _, off, k in stepping(name, step):
            stepmask[off:off + k] = True
        own = stepmask.copy()
        own[:lo] = False
        own[hi:] = False
        return stepmask, own, lo, hi

    def run(self):
        ora = oracle_run(self.adam_w, self.clip, self.bad_step)
        if self.clip is not None:
            assert all(o['coef'] < 1.0 for o in ora), 'the clip of this case must bite'
        for step in range(STEPS):
            self.step(step, ora[step])
        return self.worst

    def step(self, step, ref):
        opt, red = self.opt, self.red
        gr = gradients(step)
        masks, full = {}, {}
        for name, b in self.buckets.items():
            g = np.full(b.padded, GARBAGE, np.float32)
            g[:b.numel] = gr[name]
            masks[name] = self._own_mask(name, step)
            full[name] = g
        if step == self.bad_step:
            # one infinity, inside this rank's entries or only in what the other ranks would report
            stepmask, own, _, _ = masks['hook']
            cand = np.flatnonzero(own if self.bad_where == 'own' else stepmask & ~own)
            assert cand.size, 'no element of that kind on this rank'
            full['hook'][cand[cand.size // 2]] = np.inf
        other = 0.0
        with np.errstate(over='ignore', invalid='ignore'):
            for name, b in self.buckets.items():
                stepmask, own, lo, hi = masks[name]
                other += float((full[name][stepmask & ~own].astype(np.float64) ** 2).sum())
                b.shard32.copy_(torch.from_numpy(full[name][lo:hi]))
                b.has_grad = True
        self.buckets['hook'].had = had_at(step)
        red.other_sq, red.reduces, red.gathers = other, 0, []
        before = None
        if opt.parts is not None:
            before = [(_bits(pt.pflat), _bits(pt.m), _bits(pt.v)) for pt in opt.parts]
        versions = [p._version for ps in self.params.values() for p in ps]

        norm = opt.step(clip_grad=self.clip)

        parts = {'sink': opt.parts[0], 'hook': opt.parts[1]}
        assert parts['sink'].bucket is self.buckets['sink'] and parts['hook'].bucket is self.buckets['hook']
        if before is None:          # first step: the partition was just built; zero moments, parameters as given
            before = []
            for name in ('sink', 'hook'):
                b = self.buckets[name]
                flat = np.zeros(b.padded, np.float32)
                offs = sink_layout_offsets()[0] if name == 'sink' else hook_offsets()[0]
                for a, off in zip(initial_params()[name], offs):
                    flat[off:off + a.size] = a
                z = np.zeros(b.padded // self.world, np.int32)
                before.append((flat.view(np.int32), z, z))
        failed = []         # the value checks all run; what failed is raised together at the end of the step
        # ---- the norm and the clip
        if self.clip is None:
            assert norm is None and opt.last_ctl is None
            assert red.reduces == 0
        else:
            assert red.reduces == (1 if self.world > 1 else 0)
            ctl = opt.last_ctl.cpu().tolist()
            if ref['bad']:
                assert not np.isfinite(float(norm)) and ctl[2] == 1.0 and ctl[1] == 0.0
            else:
                assert ctl[2] == 0.0
                rn, rc = abs(float(norm) - ref['norm']) / ref['norm'], abs(ctl[1] - ref['coef']) / ref['coef']
                self._note('norm', rn / 1e-5)
                self._note('coef', rc / 1e-5)
                if not (rn <= 1e-5 and rc <= 1e-5):
                    failed.append(('norm', step, float(norm), ref['norm'], ctl[1], ref['coef']))
        # ---- the parameter all-gather: every partitioned bucket, the rank's own chunk of the output, in place
        if self.world > 1:
            assert len(red.gathers) == len(opt.parts)
            for pt, (out, src) in zip(opt.parts, red.gathers):
                assert out is pt.pflat
                assert src.data_ptr() == out.data_ptr() + 4 * pt.lo and src.numel() == pt.hi - pt.lo
        else:
            assert red.gathers == []
        # ---- values
        S = step + 1
        for (name, pt), (p0, m0, v0) in zip(parts.items(), before):
            stepmask, own, lo, hi = masks[name]
            assert (pt.lo, pt.hi, pt.padded) == (lo, hi, self.buckets[name].padded)
            p1, m1, v1 = _bits(pt.pflat), _bits(pt.m), _bits(pt.v)
            touched = np.zeros_like(own) if ref['bad'] else own
            # everything outside the stepping entries is bit-identical: other ranks' parts of pflat, layout holes, padding,
            # the parameter without a gradient and its moments; on a skipped step, everything
            if not np.array_equal(p1[~touched], p0[~touched]):
                failed.append(('untouched', name, step, 'pflat changed outside the stepping entries'))
            if not np.array_equal(m1[~touched[lo:hi]], m0[~touched[lo:hi]]):
                failed.append(('untouched', name, step, 'm changed outside the entries'))
            if not np.array_equal(v1[~touched[lo:hi]], v0[~touched[lo:hi]]):
                failed.append(('untouched', name, step, 'v changed outside the entries'))
            offs = sink_layout_offsets()[0] if name == 'sink' else hook_offsets()[0]
            pf, mf, vf = (x.view(np.float32).astype(np.float64) for x in (p1, m1, v1))
            for i, off in enumerate(offs):
                k = ref[name]['p'][i].size
                a, b_ = max(off, lo), min(off + k, hi)
                if a >= b_:
                    continue
                rp, rm, rv = (ref[name][key][i][a - off:b_ - off] for key in 'pmv')
                bound = S * (2e-6 * np.abs(ref[name]['p'][i]).max() + 1e-7)
                ep = np.abs(pf[a:b_] - rp).max()
                em = (np.abs(mf[a - lo:b_ - lo] - rm) / (1e-8 + 1e-5 * np.abs(rm))).max()
                ev = (np.abs(vf[a - lo:b_ - lo] - rv) / (1e-10 + 1e-5 * np.abs(rv))).max()
                self._note('p', ep / bound)
                self._note('m', em)
                self._note('v', ev)
                if not (ep <= bound and em <= 1.0 and ev <= 1.0):
                    failed.append(('value', name, i, step, 'parameter / exp_avg / exp_avg_sq over bound', ep / bound, em, ev))
        # ---- the parameters are still views into the flat buffers, and their version counters grew
        for name, pt in parts.items():
            offs = sink_layout_offsets()[0] if name == 'sink' else hook_offsets()[0]
            for p, off in zip(self.params[name], offs):
                assert p.data_ptr() == pt.pflat.data_ptr() + 4 * off and p.is_contiguous()
        assert all(p._version > v for v, p in zip(versions, (p for ps in self.params.values() for p in ps)))
        if failed:
            raise Broke({f[0] for f in failed}, failed[:4])


def ranks(worlds=WORLDS):
    return [(w, r) for w in worlds for r in range(w)]
