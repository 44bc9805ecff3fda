"""The HIP multi-tensor kernels (``vlmo_mt_grad_norm``, ``vlmo_mt_adam``) in the form ZeRO-2 uses them: table entries that
are slices of flat buffers, cut by parameter offsets and rank boundaries, 0 / 4 / 8 / 12 bytes off 16-byte alignment, longer
than one chunk, for every rank of W = 1, 2, 3, 8 -- the cases of tests/zero_cases.py (run on an emulation in
test_zero_slices_cpu.py), here through the real ``zero.ZeroAdam`` on the GPU, against the fp64 oracle on whole tensors.
Every launch table is bounds-checked against the optimizer's buffers before the kernel sees it.

Then ``optim.FusedAdam`` on parameters that are views 1, 2 and 3 elements into their storage (the scalar branch of
``adam_chunk``), and on an aligned parameter whose gradient is a misaligned view (the five-pointer alignment test).

Bounds: those of tests/test_optim_gpu.py (see tests/zero_cases.py)."""
import numpy as np
import pytest
import torch

from exploremultimodal_amd import mt, optim
from oracle import adamw_oracle
from tests import zero_cases as zc

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('world,rank', zc.ranks())
def test_each_rank_matches_the_whole_tensor_oracle(world, rank):
    sim = zc.Sim(world, rank, DEV, cls=zc.CheckedZero)
    try:
        sim.run()
    finally:
        print(f'\nworst error / bound, W={world} rank {rank}:', {k: round(v, 4) for k, v in sim.worst.items()})


@pytest.mark.parametrize('rank', range(3))
@pytest.mark.parametrize('variant', sorted(zc.VARIANTS))
def test_variants_at_world_3(variant, rank):
    sim = zc.Sim(3, rank, DEV, cls=zc.CheckedZero, **zc.VARIANTS[variant])
    try:
        sim.run()
    finally:
        print(f'\nworst error / bound, {variant} rank {rank}:', {k: round(v, 4) for k, v in sim.worst.items()})


# ------------------------------------------------------------------------------------------------ FusedAdam on views
GUARD = 8       # elements of storage on either side of a view; they must not change
# (start of the parameter view in its storage, start of the gradient view in its storage, elements)
VIEWS = [(1, 0, 1000), (2, 2, mt.CHUNK + 5), (3, 1, 7), (0, 1, 257), (0, 0, 33), (1, 1, 1)]
VIEW_GROUPS = [(2e-3, 0.05), (5e-4, 0.0)]


def _view(start, n, values):
    store = torch.full((GUARD + start + n + GUARD,), 7.0, device=DEV)
    assert store.data_ptr() % 16 == 0
    v = store[GUARD + start:GUARD + start + n]
    v.copy_(values)
    return store, v


@pytest.mark.parametrize('clip', [None, 0.5])
def test_fused_adam_on_misaligned_views_matches_the_oracle(clip):
    g = torch.Generator().manual_seed(21)
    stores, ps = [], []
    for ps_, _, n in VIEWS:
        store, v = _view(ps_, n, torch.randn(n, generator=g) * 0.5)
        stores.append(store)
        ps.append(torch.nn.Parameter(v))
        assert ps[-1].data_ptr() == store.data_ptr() + 4 * (GUARD + ps_)
    assert {p.data_ptr() % 16 for p in ps} == {0, 4, 8, 12}
    groups = [{'params': ps[i::2], 'lr': lr, 'weight_decay': wd} for i, (lr, wd) in enumerate(VIEW_GROUPS)]
    opt = optim.FusedAdam(groups, betas=zc.BETAS, eps=zc.EPS)
    o_p = [p.detach().cpu().double().numpy() for p in ps]
    o_m = [np.zeros_like(x) for x in o_p]
    o_v = [np.zeros_like(x) for x in o_p]
    worst = {'p': 0.0, 'm': 0.0, 'v': 0.0, 'norm': 0.0}
    for step in range(1, 4):
        grads, gstores = [], []
        for (_, gs_, n), p in zip(VIEWS, ps):
            gr = torch.randn(n, generator=g) * (0.1 * step)
            gstore, gv = _view(gs_, n, gr)
            gstores.append(gstore)
            p.grad = gv
            assert p.grad.data_ptr() == gstore.data_ptr() + 4 * (GUARD + gs_)
            grads.append(gr.numpy())
        # the mixed case: everything 16-byte aligned but the gradient
        assert ps[3].data_ptr() % 16 == 0 and ps[3].grad.data_ptr() % 16 == 4
        norm = opt.step(clip_grad=clip)
        o_norm, o_coef = adamw_oracle.clip_coef(grads, clip)
        if clip is not None:
            assert o_coef < 1.0
            worst['norm'] = max(worst['norm'], abs(norm.item() - o_norm) / o_norm / 1e-5,
                                abs(opt.last_ctl[1].item() - o_coef) / o_coef / 1e-5)
        for i, gr in enumerate(grads):
            lr, wd = VIEW_GROUPS[i % 2]
            o_p[i], o_m[i], o_v[i] = adamw_oracle.adam_step(o_p[i], gr.astype(np.float64) * o_coef, o_m[i], o_v[i], step, lr,
                                                            zc.BETAS[0], zc.BETAS[1], zc.EPS, wd)
        for i, (p, store, gstore, (ps_, gs_, n)) in enumerate(zip(ps, stores, gstores, VIEWS)):
            st = opt.state[p]
            bound = step * (2e-6 * np.abs(o_p[i]).max() + 1e-7)
            ep = np.abs(p.detach().cpu().double().numpy() - o_p[i]).max() / bound
            em = (np.abs(st['exp_avg'].cpu().double().numpy() - o_m[i]) / (1e-8 + 1e-5 * np.abs(o_m[i]))).max()
            ev = (np.abs(st['exp_avg_sq'].cpu().double().numpy() - o_v[i]) / (1e-10 + 1e-5 * np.abs(o_v[i]))).max()
            worst.update(p=max(worst['p'], ep), m=max(worst['m'], em), v=max(worst['v'], ev))
            # the storage around the views is untouched, and so is the gradient
            s = store.cpu()
            assert torch.equal(s[:GUARD + ps_], torch.full((GUARD + ps_,), 7.0))
            assert torch.equal(s[-GUARD:], torch.full((GUARD,), 7.0))
            assert torch.equal(gstore[GUARD + gs_:GUARD + gs_ + n].cpu(), torch.from_numpy(grads[i]))
    print('\nworst error / bound, FusedAdam on views, clip', clip, {k: round(v, 4) for k, v in worst.items()})
    assert worst['norm'] <= 1.0 and worst['p'] <= 1.0 and worst['m'] <= 1.0 and worst['v'] <= 1.0, worst


def test_fused_adam_counts_a_skipped_step_as_the_slice_oracle_assumes():
    """``zero_cases.oracle_run`` lets a step skipped for a non-finite gradient count for the bias corrections, because
    ``optim.FusedAdam`` does (its host-side counters are not counted back); ZeroAdam is held to that oracle in the cases
    above, this holds FusedAdam to it."""
    g = torch.Generator().manual_seed(22)
    ps = [torch.nn.Parameter((torch.randn(n, generator=g) * 0.5).to(DEV)) for n in (300, 17)]
    before = [p.detach().cpu().double().numpy() for p in ps]
    opt = optim.FusedAdam(ps, lr=2e-3, betas=zc.BETAS, eps=zc.EPS, weight_decay=0.05)
    for p in ps:
        p.grad = torch.ones_like(p)
    ps[1].grad[3] = float('inf')
    opt.step(clip_grad=0.5)
    assert opt.last_ctl[2].item() == 1.0 and all(np.array_equal(p.detach().cpu().double().numpy(), b) for p, b in zip(ps, before))
    grads = [(torch.randn(p.shape, generator=g) * 0.1) for p in ps]
    for p, gr in zip(ps, grads):
        p.grad = gr.to(DEV)
    opt.step(clip_grad=0.5)
    _, coef = adamw_oracle.clip_coef([gr.numpy() for gr in grads], 0.5)
    for p, b, gr in zip(ps, before, grads):
        z = np.zeros_like(b)
        counted, _, _ = adamw_oracle.adam_step(b, gr.double().numpy() * coef, z, z, 2, 2e-3, *zc.BETAS, zc.EPS, 0.05)
        not_counted, _, _ = adamw_oracle.adam_step(b, gr.double().numpy() * coef, z, z, 1, 2e-3, *zc.BETAS, zc.EPS, 0.05)
        bound = 2e-6 * np.abs(counted).max() + 1e-7
        got = p.detach().cpu().double().numpy()
        assert np.abs(got - counted).max() <= bound
        assert np.abs(got - not_counted).max() > 100 * bound        # the two rules are far apart: the check can tell them
        assert int(opt.state[p]['step']) == 2


def test_the_norm_does_not_depend_on_table_order_or_alignment():
    """The same tensors, cut into the same chunks, listed in another order and with gradients 0, 4 or 12 bytes off 16-byte
    alignment (the scalar load path), must give the same norm and clip coefficient to the bit: one ulp between two
    coefficients is one ulp on every weight, and the next gradients of a bf16 model move by far more than run-to-run noise
    for it (profiles/r11_zero_slices_measurements.txt).  ``vlmo_mt_grad_norm`` squares and sums in double and rounds each
    chunk once; with its earlier fp32 sums the orders below disagree in the last bit (third gradient set)."""
    sizes = [300 * 257, 1000, mt.CHUNK + 3, 7, 64 * 3 * 16 * 16, 1, 2 * mt.CHUNK, 33, 70001]
    g = torch.Generator().manual_seed(23)
    for trial in range(8):
        grads = [torch.randn(n, generator=g) * 0.1 for n in sizes]
        seen = []
        for order, start in ((range(len(sizes)), 0), (reversed(range(len(sizes))), 1), ([3, 8, 0, 5, 2, 7, 1, 6, 4], 3)):
            ps, keep = [], []
            for i in order:
                p = torch.nn.Parameter(torch.zeros(sizes[i], device=DEV))
                store, gv = _view(start, sizes[i], grads[i])
                keep.append(store)
                p.grad = gv
                ps.append(p)
            opt = optim.FusedAdam(ps, lr=1e-3)
            opt.step(clip_grad=1.0)
            seen.append(opt.last_ctl[:3].cpu().clone())
        assert seen[0][2] == 0 and seen[0][1] < 1.0
        assert torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2]), (trial, [s.tolist() for s in seen])


def test_zero_adam_and_fused_adam_report_the_same_norm_at_world_1():
    """At world size 1 every ZeroAdam entry is a whole parameter, so both optimizers cut the same chunks; ZeroAdam lists
    them bucket by bucket, at the offsets of its flat buffers (most of them misaligned), squares the kernel's norm and
    takes the root again in torch.  Same gradients -> the same norm, coefficient and flag, bit for bit, in each of the
    three steps of the main case.  (Above world size 1 the slices cut other chunks and the ranks' squares are added in
    fp32: no such claim.)"""
    sim = zc.Sim(1, 0, DEV, cls=zc.CheckedZero)
    ora = zc.oracle_run(True, 1.0, None)
    for step in range(zc.STEPS):
        sim.step(step, ora[step])
        zero = sim.opt.last_ctl[:3].cpu().clone()
        gr, ps = zc.gradients(step), []
        for name in ('hook', 'sink'):           # the other bucket first, every gradient in an allocation of its own
            for _, off, n in zc.stepping(name, step):
                p = torch.nn.Parameter(torch.zeros(n, device=DEV))
                p.grad = torch.from_numpy(gr[name][off:off + n].copy()).to(DEV)
                ps.append(p)
        fused = optim.FusedAdam(ps, lr=1e-3)
        fused.step(clip_grad=1.0)
        assert torch.equal(zero, fused.last_ctl[:3].cpu()), (step, zero.tolist(), fused.last_ctl[:3].tolist())
