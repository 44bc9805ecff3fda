"""Host logic of engine.StackFn that needs no GPU: the split of a block's parameter list into its groups
(engine.block_groups / group_numel / group_layout), which must agree with what engine._fill_grads carves, and the
choice of a group's gradient bucket on the local route (engine._local_bucket), one case per outcome."""
import pytest
import torch

from exploremultimodal_amd import engine

D, HID = 8, 32


def _block(nexp):
    mk = lambda *shape: torch.nn.Parameter(torch.zeros(*shape))
    shared = [mk(D), mk(D), mk(D), mk(D), mk(3 * D, D), mk(D), mk(D), mk(D, D), mk(D), mk(D), mk(D)]
    experts = [[mk(HID, D), mk(HID), mk(D, HID), mk(D)] for _ in range(nexp)]
    return shared, experts


class _Desc:                    # stands in for the ctypes descriptor: accepts attribute and indexed writes
    def __init__(self, nexp):
        for n in ('dw1', 'db1', 'dw2', 'db2'):
            object.__setattr__(self, n, [0] * nexp)


@pytest.mark.parametrize('nexp', [1, 2, 3])
def test_block_groups_agree_with_the_carved_gradients(nexp):
    shared, experts = _block(nexp)
    bp = shared + [p for e in experts for p in e]
    groups = engine.block_groups(bp)
    assert len(groups) == 1 + nexp
    # groups and spans: shared first, then one per expert, tiling the block list in order
    assert (groups[0].lo, groups[0].hi) == (0, engine.N_SHARED) == (0, len(shared))
    for e, g in enumerate(groups[1:]):
        assert (g.lo, g.hi) == (len(shared) + engine.N_EXPERT * e, len(shared) + engine.N_EXPERT * (e + 1))
    for g in groups:
        assert len(g.params) == g.hi - g.lo and all(a is b for a, b in zip(g.params, bp[g.lo:g.hi]))
    assert groups[-1].hi == len(bp)
    # the named weight positions
    assert groups[0].params[engine.QKV_W].shape == (3 * D, D) and groups[0].params[engine.PROJ_W].shape == (D, D)
    for g in groups[1:]:
        assert g.params[engine.FC1_W].shape == (HID, D) and g.params[engine.FC2_W].shape == (D, HID)
    assert engine._group_key(groups[0].params) == shared[4].data_ptr()
    assert [engine._group_key(g.params) for g in groups[1:]] == [e[0].data_ptr() for e in experts]
    # sizes: every parameter plus, in the shared bucket, the k-bias hole between q_bias and v_bias
    sizes = [engine.group_numel(g, D, HID) for g in groups]
    assert sizes[0] == sum(p.numel() for p in shared) + D
    assert sizes[1:] == [sum(p.numel() for p in e) for e in experts]
    # layouts: the dispatch, and the offsets against the gradients _fill_grads carves out of buckets of these sizes
    g1, g2, n1w, n1b, qkv_w, q_bias, v_bias, proj_w, proj_b, n2w, n2b = shared
    o = 6 * D + 4 * D * D
    want = [(g1, 0), (g2, D), (n1w, 2 * D), (n1b, 3 * D), (n2w, 4 * D), (n2b, 5 * D), (qkv_w, 6 * D),
            (proj_w, 6 * D + 3 * D * D), (proj_b, o), (q_bias, o + D), (v_bias, o + 3 * D)]
    got = engine.group_layout(groups[0], D, HID)
    assert [(id(p), off) for p, off in got] == [(id(p), off) for p, off in want]
    for g, (w1, b1, w2, b2) in zip(groups[1:], experts):
        want = [(w1, 0), (b1, HID * D), (w2, HID * D + HID), (b2, 2 * HID * D + HID)]
        assert [(id(p), off) for p, off in engine.group_layout(g, D, HID)] == [(id(p), off) for p, off in want]
    flats = [torch.arange(n, dtype=torch.float32) + 10000 * gi for gi, n in enumerate(sizes)]
    grads = engine._fill_grads(_Desc(nexp), flats, D, HID, nexp)
    assert len(grads) == len(bp)
    for gi, g in enumerate(groups):
        offs = {id(p): off for p, off in engine.group_layout(g, D, HID)}
        assert len(offs) == len(g.params)
        for p, gr in zip(g.params, grads[g.lo:g.hi]):
            assert gr.shape == p.shape
            assert gr.reshape(-1)[0].item() == 10000.0 * gi + offs[id(p)]       # the bucket holds arange: first element = offset
            assert offs[id(p)] + p.numel() <= sizes[gi]


@pytest.mark.parametrize('n', [0, 10, 12, 14, 16])
def test_block_groups_refuses_other_lengths(n):
    with pytest.raises(ValueError):
        engine.block_groups([torch.zeros(1)] * n)


def _hold_views(g, foreign=None):
    """.grad of the group's parameters = this layout's views of one flat buffer, as an earlier backward leaves them."""
    n = engine.group_numel(g, D, HID)
    flat = torch.zeros(n + 8)[4:4 + n]
    for p, off in engine.group_layout(g, D, HID):
        p.grad = flat[off:off + p.numel()].view(p.shape)
    if foreign is not None:     # one parameter holds a gradient of its own (set_to_none + another producer)
        g.params[foreign].grad = torch.zeros_like(g.params[foreign])
    return flat


@pytest.mark.parametrize('which', [0, 1])
def test_local_bucket_outcomes(which):
    """which: the shared group / an expert group."""
    def group():
        shared, experts = _block(2)
        return engine.block_groups(shared + [p for e in experts for p in e])[which * 2]

    def fresh_fn(g):
        made = []

        def fresh():
            made.append(torch.empty(engine.group_numel(g, D, HID)))
            return made[-1]
        return fresh, made

    def choose(g, wanted=True, reg=None, permitted=frozenset(), into_grad=False):
        fresh, made = fresh_fn(g)
        flat, how = engine._local_bucket(g, D, HID, wanted, reg, permitted, into_grad, fresh)
        return flat, how, made

    # an earlier node of the task registered a buffer: that buffer, nothing allocated
    g = group()
    key = engine._group_key(g.params)
    earlier = torch.zeros(engine.group_numel(g, D, HID))
    reg = {key: earlier}
    flat, how, made = choose(g, reg=reg, permitted=frozenset([key]), into_grad=True)
    assert flat is earlier and how == engine.FROM_TASK and not made and reg == {key: earlier}

    # existing .grad views accepted
    g = group()
    held = _hold_views(g)
    flat, how, made = choose(g, into_grad=True)
    assert how == engine.FROM_GRAD and not made
    assert flat.data_ptr() == held.data_ptr() and flat.numel() == held.numel()
    # ... a frozen parameter of the group need not hold one
    g = group()
    held = _hold_views(g)
    g.params[1].requires_grad_(False)
    g.params[1].grad = None
    assert choose(g, into_grad=True)[1] == engine.FROM_GRAD
    # ... but only inside accumulate_into_grad()
    g = group()
    _hold_views(g)
    flat, how, made = choose(g, into_grad=False)
    assert how == engine.FRESH and flat is made[0]

    # existing .grad views rejected because of a hook (it must see this pass's gradient)
    for hook in ('tensor', 'post'):
        g = group()
        _hold_views(g)
        if hook == 'tensor':
            g.params[2].register_hook(lambda gr: gr)
        else:
            g.params[2].register_post_accumulate_grad_hook(lambda p: None)
        flat, how, made = choose(g, into_grad=True)
        assert how == engine.FRESH and flat is made[0], hook

    # existing .grad views rejected because the base is foreign
    for foreign in (0, -1):
        g = group()
        _hold_views(g, foreign=foreign)
        flat, how, made = choose(g, into_grad=True)
        assert how == engine.FRESH and flat is made[0], foreign
    g = group()
    for p in g.params:          # plain gradients, no common flat buffer at all
        p.grad = torch.zeros_like(p)
    assert choose(g, into_grad=True)[1] == engine.FRESH

    # fresh and registered: the walk permitted the group
    g = group()
    key = engine._group_key(g.params)
    reg = {}
    flat, how, made = choose(g, reg=reg, permitted=frozenset([key]))
    assert how == engine.FRESH and flat is made[0] and reg == {key: flat}

    # fresh but not permitted: another op produces a gradient for the group, later nodes must not add into this buffer
    g = group()
    reg = {}
    flat, how, made = choose(g, reg=reg, permitted=frozenset([engine._group_key(g.params) + 4]))
    assert how == engine.FRESH and flat is made[0] and reg == {}
    # ... or the node is outside the walk (no registry)
    assert choose(g, reg=None, permitted=frozenset([engine._group_key(g.params)]))[1] == engine.FRESH

    # not wanted (the task asks for part of the group only): fresh, never registered, never an earlier buffer or .grad
    g = group()
    key = engine._group_key(g.params)
    _hold_views(g)
    reg = {key: torch.zeros(engine.group_numel(g, D, HID))}
    before = dict(reg)
    flat, how, made = choose(g, wanted=False, reg=reg, permitted=frozenset([key]), into_grad=True)
    assert how == engine.FRESH and flat is made[0] and reg == before
    reg = {}
    assert choose(g, wanted=False, reg=reg, permitted=frozenset([key]))[1] == engine.FRESH and reg == {}
