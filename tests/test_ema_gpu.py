"""Weight average on the device: vlmo_mt_ema and vlmo_mt_adam_ema against the fp64 recurrence e + w (p - e), the AdamW
step with the average folded in against the step followed by the update (bit for bit), and ema.ModelEma behind the
training step of the module -- where a missing version bump would leave ema.module running on stale bf16 weight shadows.

Bound against the recurrence (tests/test_ema_cpu.py derives it): 3 S 2^-24 max(|e|, |p|) per element over S updates."""
import copy
import ctypes
import os

import pytest
import torch

from exploremultimodal_amd import hip, optim
from exploremultimodal_amd.build import build_model
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
# one element .. three chunks of 65536, a chunk exactly, a chunk and a scalar tail; the last tensor is a view that starts one
# element into its storage (4 bytes off the 16-byte alignment: the scalar path), long enough to cross a chunk boundary
SIZES = [1, 3, 4, 1023, 65536, 65539, 131073]
UNALIGNED = 70001


def _ema_mod():
    from exploremultimodal_amd import ema
    return ema


def _tensors(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    ts = [(torch.randn(n, generator=g) * scale).to(DEV) for n in SIZES]
    ts.append((torch.randn(UNALIGNED + 1, generator=g) * scale).to(DEV)[1:])
    assert ts[-1].data_ptr() % 16 == 4 and all(t.data_ptr() % 16 == 0 for t in ts[:-1])
    return ts


def _bound(steps, *tensors):
    big = tensors[0].abs().double()
    for t in tensors[1:]:
        big = torch.maximum(big, t.abs().double())
    return 3 * steps * 2.0 ** -24 * big


@pytest.mark.parametrize('w', [1e-4, 0.1, 0.5, 0.9])
def test_mt_ema_matches_the_fp64_recurrence(w):
    ema = _ema_mod()
    es, ps = _tensors(0), _tensors(1)
    e0 = [e.clone() for e in es]
    p0 = [p.clone() for p in ps]
    tl, keep = ema.tensor_list(torch.device(DEV, 0), list(zip(es, ps)))
    assert tl.n_chunks == 1 + 1 + 1 + 1 + 1 + 2 + 3 + 2
    hip.mt_ema(tl, w)
    torch.cuda.synchronize()
    for i, (e, a, p) in enumerate(zip(es, e0, ps)):
        assert torch.equal(p, p0[i])                                           # the source is only read
        ref = a.double() + w * (p.double() - a.double())
        err = (e.double() - ref.float().double()).abs()
        assert (err <= _bound(1, a, p)).all(), (i, err.max().item())
        assert not torch.equal(e, a)


def test_mt_ema_edges():
    ema = _ema_mod()
    es, ps = _tensors(2), _tensors(3, scale=1e-3)          # |p| << |e|: (p - e) + e would not give p back
    e0 = [e.clone() for e in es]
    dev = torch.device(DEV, 0)
    tl, keep = ema.tensor_list(dev, list(zip(es, ps)))
    hip.mt_ema(tl, 0.0)
    for e, a in zip(es, e0):
        assert torch.equal(e, a)
    with pytest.raises(RuntimeError, match=r'vlmo_mt_ema.*outside \[0, 1\]'):
        hip.mt_ema(tl, 1.5)
    for e, a in zip(es, e0):
        assert torch.equal(e, a)
    hip.mt_ema(tl, 1.0)
    for e, p in zip(es, ps):
        assert torch.equal(e, p)
    # the fixed point: an average equal to its source stays put whatever w
    for w in (1e-4, 0.3, 0.7):
        hip.mt_ema(tl, w)
    for e, p in zip(es, ps):
        assert torch.equal(e, p)
    empty, keep2 = ema.tensor_list(dev, [])
    assert empty.n_chunks == 0
    assert hip.lib().vlmo_mt_ema(ctypes.byref(empty), 0.1, torch.cuda.current_stream().cuda_stream) == 0


class _Bag(torch.nn.Module):
    """The tensors of SIZES (+ the unaligned view) as parameters, one parameter no optimizer holds, one frozen one, a
    float and an integer buffer."""

    def __init__(self, seed):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t) for t in _tensors(seed, 0.5)])
        g = torch.Generator().manual_seed(seed + 50)
        self.outside = torch.nn.Parameter(torch.randn(777, generator=g).to(DEV))
        self.frozen = torch.nn.Parameter(torch.randn(100, generator=g).to(DEV), requires_grad=False)
        self.register_buffer('stat', torch.randn(33, generator=g).to(DEV))
        self.register_buffer('count', torch.zeros((), dtype=torch.int64, device=DEV))


def _run(fused, grads_of_step, steps=3, decay=0.9, clip=1.0):
    ema = _ema_mod()
    net = _Bag(7)
    avg = ema.ModelEma(net, decay=decay)
    opt = optim.FusedAdam([{'params': list(net.ps)[:4], 'lr': 2e-3, 'weight_decay': 0.05},
                           {'params': list(net.ps)[4:], 'lr': 5e-4, 'weight_decay': 0.0}], betas=(0.9, 0.98))
    trace = []
    for s in range(steps):
        for i, p in enumerate(net.ps):
            p.grad = grads_of_step(s, i, p)
        with torch.no_grad():           # what an optimizer never sees still moves: the average must follow it
            net.outside.add_(0.25)
            net.stat.mul_(1.5)
            net.count.add_(2)
        before = {k: v.clone() for k, v in avg.state_dict().items()}
        if fused:
            opt.step(clip_grad=clip, ema=avg)
        else:
            opt.step(clip_grad=clip)
            avg.update(net)
        trace.append((before, {k: v.clone() for k, v in net.state_dict().items()}, opt.last_ctl.clone()))
    torch.cuda.synchronize()
    return net, avg, opt, trace


def test_fused_step_equals_step_then_update_bit_for_bit():
    def grads(s, i, p):
        if s == 1 and i == 3:
            return None                 # no gradient in step 2: the standalone path, and its step counter falls behind
        g = torch.Generator().manual_seed(1000 * s + i)
        return (torch.randn(p.shape, generator=g) * 0.3).to(DEV)

    n1, a1, o1, t1 = _run(True, grads)
    n2, a2, o2, t2 = _run(False, grads)
    assert [int(o1.state[p]['step']) for p in n1.ps] == [3, 3, 3, 2, 3, 3, 3, 3]
    for k, v in n1.state_dict().items():
        assert torch.equal(v, n2.state_dict()[k]), k
    for p, q in zip(n1.ps, n2.ps):
        assert torch.equal(o1.state[p]['exp_avg'], o2.state[q]['exp_avg'])
        assert torch.equal(o1.state[p]['exp_avg_sq'], o2.state[q]['exp_avg_sq'])
    for k, v in a1.state_dict().items():
        assert torch.equal(v, a2.state_dict()[k]), k
    # ... and both are the recurrence over the parameter values after each step (S = 3), not merely each other
    w = 1.0 - a1.decay
    ref = {k: v.double() for k, v in t1[0][0].items()}
    big = {k: v.abs().double() for k, v in t1[0][0].items()}
    for _, after, ctl in t1:
        assert ctl[2].item() == 0.0 and 0.0 < ctl[1].item() < 1.0        # the clip is live
        for k, p in after.items():
            if p.is_floating_point():
                ref[k] = ref[k] + w * (p.double() - ref[k])
                big[k] = torch.maximum(big[k], torch.maximum(ref[k].abs(), p.abs().double()))
    for k, v in a1.state_dict().items():
        if v.is_floating_point():
            err = (v.double() - ref[k].float().double()).abs()
            assert (err <= 3 * 3 * 2.0 ** -24 * big[k]).all(), (k, err.max().item())
            if k != 'frozen':
                assert not torch.equal(v, n1.state_dict()[k]), k
        else:
            assert torch.equal(v, n1.state_dict()[k]) and v.item() == 6
    assert torch.equal(a1.state_dict()['frozen'], n1.frozen)             # never moved: the fixed point


def test_skipped_step_still_moves_the_average():
    def grads(s, i, p):
        g = torch.ones_like(p)
        if s == 1 and i == 5:
            g[65537] = float('inf')
        return g

    runs = [_run(fused, grads, steps=2) for fused in (True, False)]
    for net, avg, opt, trace in runs:
        (_, after0, ctl0), (before1, after1, ctl1) = trace
        assert ctl0[2].item() == 0.0 and ctl1[2].item() == 1.0
        for i, p in enumerate(net.ps):
            assert torch.equal(p, after0[f'ps.{i}'])                     # parameters and moments of step 1 stand
            m = opt.state[p]['exp_avg']
            assert torch.isfinite(m).all() and torch.isfinite(opt.state[p]['exp_avg_sq']).all()
        w = 1.0 - avg.decay
        for k, e in avg.state_dict().items():
            if e.is_floating_point():
                ref = before1[k].double() + w * (after1[k].double() - before1[k].double())
                err = (e.double() - ref.float().double()).abs()
                assert (err <= _bound(1, before1[k], after1[k])).all(), (k, err.max().item())
        assert not torch.equal(avg.state_dict()['ps.5'], before1['ps.5'])
    (n1, a1, o1, _), (n2, a2, o2, _) = runs
    for k, v in a1.state_dict().items():
        assert torch.equal(v, a2.state_dict()[k]), k
    for p, q in zip(n1.ps, n2.ps):
        assert torch.equal(p, q) and torch.equal(o1.state[p]['exp_avg'], o2.state[q]['exp_avg'])
        assert torch.equal(o1.state[p]['exp_avg_sq'], o2.state[q]['exp_avg_sq'])


def _mini():
    cfg = synth.make_config('mini', loss_names=['itc', 'mlm'], drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0)
    torch.manual_seed(0)
    model = build_model(cfg).to(DEV).train()
    batch = {k: v.to(DEV) for k, v in synth.synth_batch(cfg.model, 2, seed=3).items()}
    return cfg, model, batch


def _close(got, ref):
    """The bound the mini backbone tests hold the engine's output to (tests/test_backbone_gpu.py)."""
    return ((got - ref).abs() <= 2e-2 + 2e-2 * ref.abs()).all().item()


def test_module_level_average_and_no_stale_weight_shadows():
    ema = _ema_mod()
    cfg, model, batch = _mini()
    avg = ema.ModelEma(model, decay=0.5)
    assert avg.module.transformer._shadows is not model.transformer._shadows
    assert all(b._owner() is avg.module.transformer for b in avg.module.transformer.blocks)
    assert avg.module.mlm_head.decoder.weight is avg.module.transformer.txt_embeddings.word_embeddings.weight
    # a large step, so that weights of the previous average are far outside the forward's tolerance
    opt = optim.FusedAdam([p for p in model.parameters() if p.requires_grad], lr=2e-2, betas=(0.9, 0.98))
    scaler = optim.NativeScalerWithGradNormCount()
    infer = lambda m: m.infer(dict(batch), infer_mode='img-txt')['co_feats'].detach().clone()
    ref = {k: v.double().clone() for k, v in avg.state_dict().items()}
    big = {k: v.abs().double() for k, v in avg.state_dict().items()}
    outs = []
    for step in range(2):
        with torch.no_grad():
            outs.append(infer(avg.module))              # a forward before the update: the shadows exist and can go stale
        ret = model(dict(batch))
        loss = sum(v for k, v in ret.items() if 'task_loss' in k)
        # a micro-step leaves the average alone
        held = {k: v.clone() for k, v in avg.state_dict().items()}
        if step == 0:
            scaler(loss * 0.5, opt, clip_grad=5.0, parameters=model.parameters(), update_grad=False, model_ema=avg)
            assert all(torch.equal(v, held[k]) for k, v in avg.state_dict().items())
            ret = model(dict(batch))
            loss = sum(v for k, v in ret.items() if 'task_loss' in k) * 0.5
        norm = scaler(loss, opt, clip_grad=5.0, parameters=model.parameters(), model_ema=avg)
        opt.zero_grad(set_to_none=True)
        assert torch.isfinite(norm).item()
        for k, p in model.state_dict().items():
            if p.is_floating_point():
                ref[k] = ref[k] + 0.5 * (p.double() - ref[k])
                big[k] = torch.maximum(big[k], torch.maximum(ref[k].abs(), p.abs().double()))
    for k, v in avg.state_dict().items():
        err = (v.double() - ref[k].float().double()).abs()
        assert (err <= 3 * 2 * 2.0 ** -24 * big[k]).all(), (k, err.max().item())
    with torch.no_grad():
        after = infer(avg.module)
        torch.manual_seed(5)
        fresh = build_model(cfg).to(DEV).eval()
        fresh.load_state_dict(avg.state_dict())
        want = infer(fresh)
    assert torch.isfinite(want).all()
    assert _close(after, want), (after - want).abs().max().item()
    assert not _close(outs[1], want), 'the step was too small for this test to see a stale shadow'
    assert not torch.equal(after, outs[1])


def test_other_optimizers_update_after_their_step():
    ema = _ema_mod()
    net = _Bag(9)
    avg = ema.ModelEma(net, decay=0.75)
    opt = torch.optim.SGD(list(net.ps), lr=0.1)
    e0 = {k: v.clone() for k, v in avg.state_dict().items()}
    loss = sum((p * p).sum() for p in net.ps)
    optim.NativeScalerWithGradNormCount()(loss, opt, clip_grad=None, parameters=list(net.ps), model_ema=avg)
    for k, e in avg.state_dict().items():
        p = net.state_dict()[k]
        ref = e0[k].double() + 0.25 * (p.double() - e0[k].double())
        assert ((e.double() - ref.float().double()).abs() <= _bound(1, e0[k], p)).all(), k
    assert not torch.equal(avg.state_dict()['ps.4'], e0['ps.4'])


def test_zero_adam_updates_the_average_after_the_all_gather():
    import torch.distributed as dist
    from exploremultimodal_amd.dp import GradReducer
    from exploremultimodal_amd.zero import ZeroAdam
    ema = _ema_mod()
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='29553')
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    red = None
    try:
        cfg, model, batch = _mini()
        avg = ema.ModelEma(model, decay=0.9)
        red = GradReducer(model, reduce_scatter=True, comm_dtype=torch.float32)
        groups = optim.get_parameter_groups(model, base_lr=1e-3, lr_mult_head=5, lr_mult_fusion=2, weight_decay=0.05,
                                            skip_list=model.no_weight_decay())
        opt = ZeroAdam(red, groups, betas=(0.9, 0.98), eps=1e-6)
        e0 = copy.deepcopy(avg.state_dict())
        p0 = {k: v.clone() for k, v in model.state_dict().items()}
        ret = model(dict(batch))
        loss = sum(v for k, v in ret.items() if 'task_loss' in k)
        red.prepare(loss)
        loss.backward()
        red.finish()
        norm = opt.step(clip_grad=1.0, ema=avg)
        torch.cuda.synchronize()
        assert torch.isfinite(norm).item()
        moved = 0
        for k, e in avg.state_dict().items():
            p = model.state_dict()[k]
            ref = e0[k].double() + 0.1 * (p.double() - e0[k].double())
            err = (e.double() - ref.float().double()).abs()
            assert (err <= _bound(1, e0[k], p)).all(), (k, err.max().item())
            moved += int(not torch.equal(p, p0[k]) and not torch.equal(e, e0[k]))
        assert moved > 20
    finally:
        if red is not None:
            red.close()
        dist.destroy_process_group()
