"""Host logic of the in-place accumulation gate (engine.inplace_passes / sole_producer_groups) on CPU: toy
autograd.Function stand-ins for StackFn carry `grad_groups` like the real node, and ToyStack follows the engine's
protocol -- the first permitted node of a graph task registers its gradient buffer, later ones add into it and return
None.  The walk must permit exactly the groups whose trainable parameters get their gradient from engine nodes alone;
with a foreign producer (regulariser, reused weight, an engine node without grad_groups) the group must fall back to fresh gradients, and
the gradients must come out as autograd's sum in every case."""
import torch

from exploremultimodal_amd import engine


class ToyStack(torch.autograd.Function):
    """y = x * sum(w) for a one-group 'stack'; d/dw_i = sum(dy * x).  Mirrors StackFn.backward's use of the permit."""

    @staticmethod
    def forward(ctx, x, key, *params):
        ctx.save_for_backward(x)
        ctx.key = key
        ctx.grad_groups = [(key, tuple(params))]
        return x * sum(p.sum() for p in params)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        s = (dy * x).sum()
        n = len(ctx.grad_groups[0][1])
        reg = engine._task_flats(ctx)
        ws = sum(p.sum() for p in ctx.grad_groups[0][1]).detach()
        if reg is not None and ctx.key in reg:
            reg[ctx.key].add_(s)                            # a later node: add into the registered buffer
            return (dy * ws, None) + (None,) * n
        flat = torch.full((n,), s.item())
        if reg is not None and ctx.key in engine._TASK_FLATS['groups']:
            reg[ctx.key] = flat
        return (dy * ws, None) + tuple(flat[i:i + 1].view(()) for i in range(n))


class ToyBlock(torch.autograd.Function):
    """A cooperating-but-unwalked engine node: fresh gradients, no grad_groups (stands in for any engine node that
    does not carry them)."""

    @staticmethod
    def forward(ctx, x, *params):
        ctx.save_for_backward(x, *params)
        return x * sum(p.sum() for p in params)

    @staticmethod
    def backward(ctx, dy):
        x, *params = ctx.saved_tensors
        s = (dy * x).sum()
        return (dy * sum(p.sum() for p in params),) + tuple(torch.full((), s.item()) for _ in params)


def _params(n=2, val=1.0):
    return [torch.nn.Parameter(torch.tensor(val)) for _ in range(n)]


def _grads(loss_fn, params, inplace, registered=None):
    """Gradients of loss_fn(); `registered` (a set) receives the group keys that got an in-place buffer."""
    for p in params:
        p.grad = None
    loss = loss_fn()
    if inplace:
        with engine.inplace_passes(loss):
            loss.backward()
            if registered is not None:
                registered.update(engine._TASK_FLATS['flats'])
    else:
        loss.backward()
    return [p.grad.clone() for p in params]


def test_engine_only_loss_is_permitted_for_every_group():
    a, b = _params(), _params()
    x = torch.ones(3)
    y1 = ToyStack.apply(x, 'A', *a)
    y2 = ToyStack.apply(y1, 'B', *b)
    y3 = ToyStack.apply(x, 'A', *a)              # a second pass over group A
    nodes, groups = engine.sole_producer_groups([y2.sum() + y3.sum()])
    assert groups == {'A', 'B'}
    assert nodes == {y1.grad_fn, y2.grad_fn, y3.grad_fn}


def test_foreign_producers_switch_off_exactly_the_affected_groups():
    a, b, c = _params(), _params(), _params()
    x = torch.ones(3)

    def passes():
        return ToyStack.apply(ToyStack.apply(x, 'A', *a), 'B', *b).sum() + ToyStack.apply(x, 'A', *a).sum() \
            + ToyStack.apply(x, 'C', *c).sum()
    # regulariser on one parameter of A
    assert engine.sole_producer_groups([passes() + 0.5 * a[1].pow(2)])[1] == {'B', 'C'}
    # B's weight reused outside the engine (order of the terms does not matter to the walk)
    assert engine.sole_producer_groups([(x * b[0]).square().mean() + passes()])[1] == {'A', 'C'}
    # a pass over C by an engine node without grad_groups
    assert engine.sole_producer_groups([passes() + ToyBlock.apply(x, *c).sum()])[1] == {'A', 'B'}
    # a foreign use of a FROZEN parameter produces no gradient: the group stays permitted
    c[0].requires_grad_(False)
    assert engine.sole_producer_groups([passes() + c[0] * 3.0])[1] == {'A', 'B', 'C'}
    c[0].requires_grad_(True)
    # a parameter that two groups share (the gamma stand-in case) disqualifies both
    shared = torch.nn.Parameter(torch.tensor(1.0))
    loss = ToyStack.apply(x, 'D', shared, a[0]).sum() + ToyStack.apply(x, 'E', shared, b[0]).sum()
    assert engine.sole_producer_groups([loss])[1] == frozenset()
    # a tensor hook does not produce a gradient: it sees the buffer's sum when AccumulateGrad runs
    h = a[0].register_hook(lambda g: 2 * g)
    try:
        assert engine.sole_producer_groups([passes()])[1] == {'A', 'B', 'C'}
    finally:
        h.remove()


def test_protocol_with_a_regulariser_gives_autograds_sum():
    """The ADVICE case on the toy protocol: two passes over one group plus c * w^2.  Ungated, the second pass adds
    into a buffer the input buffer no longer holds when the regulariser's gradient arrives first (w.grad 4 where 5 is
    expected); gated, it matches autograd's sum in both term orders and registers no buffer."""
    w = _params(1)
    x = torch.ones(1)
    two = lambda: ToyStack.apply(x, 'A', *w).sum() + ToyStack.apply(x, 'A', *w).sum()
    for loss_fn in (lambda: two() + 1.5 * w[0].pow(2), lambda: 1.5 * w[0].pow(2) + two()):
        ref = _grads(loss_fn, w, inplace=False)
        assert ref[0].item() == 5.0
        reg = set()
        assert _grads(loss_fn, w, inplace=True, registered=reg)[0].item() == 5.0
        assert reg == set()
    # engine-only: the in-place path runs (one registered buffer) and gives the same sum
    reg = set()
    assert _grads(two, w, inplace=True, registered=reg)[0].item() == 2.0
    assert reg == {'A'}
    assert engine._TASK_FLATS['flats'] == {}                # released with the context


def test_permit_binds_to_one_graph_task_and_ends_with_the_context():
    w = _params(1)
    x = torch.ones(1)
    loss = ToyStack.apply(x, 'A', *w).sum() + ToyStack.apply(x, 'A', *w).sum()
    with engine.inplace_passes(loss):
        loss.backward(retain_graph=True)
        first = dict(engine._TASK_FLATS['flats'])
        assert set(first) == {'A'}
        loss.backward(retain_graph=True)             # a second graph task: fresh gradients, autograd adds
        assert engine._TASK_FLATS['flats'] == first
    assert w[0].grad.item() == 4.0
    assert engine._TASK_FLATS['nodes'] is None       # no permit outside the context
    loss.backward()
    assert w[0].grad.item() == 6.0
    # autograd.grad under the permit leaves .grad alone and returns the sum
    w[0].grad = None
    loss = ToyStack.apply(x, 'A', *w).sum() + 2.0 * ToyStack.apply(x, 'A', *w).sum()
    with engine.inplace_passes(loss):
        (g,) = torch.autograd.grad(loss, w)
    assert g.item() == 3.0 and w[0].grad is None


def test_disabled_permit_and_kill_switch():
    w = _params(1)
    x = torch.ones(1)
    loss = ToyStack.apply(x, 'A', *w).sum() + ToyStack.apply(x, 'A', *w).sum()
    old = engine.INPLACE_ACCUM
    try:
        engine.INPLACE_ACCUM = False
        with engine.inplace_passes(loss):
            assert engine._TASK_FLATS['nodes'] is None
    finally:
        engine.INPLACE_ACCUM = old
    with engine.inplace_passes(loss, enabled=False):
        assert engine._TASK_FLATS['nodes'] is None
        loss.backward()
    assert w[0].grad.item() == 2.0
