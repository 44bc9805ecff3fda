"""The gradient reducer declares its state: every attribute of a GradReducer and of its buckets exists once the
constructor has run, two steps through the public protocol add none, and neither dp.py nor zero.py probes an object
with a defaulted getattr or a hasattr (a mistyped name there is silently the default)."""
import ast
import os

import pytest
import torch
import torch.distributed as dist
import torch.nn as nn

from .test_dp_gloo import _FakeEngineFn, _free_port


class Two(nn.Module):
    """One parameter group inside `blocks.0.` (fed through the engine-sink protocol below) and one outside it (hook path)."""

    def __init__(self):
        super().__init__()
        self.blocks = nn.ModuleList([nn.Linear(4, 4)])
        self.head = nn.Linear(4, 2)


@pytest.fixture(scope='module')
def gloo_rank0():
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()))
    dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


def _slots(obj):
    return [s for c in type(obj).__mro__ for s in c.__dict__.get('__slots__', ())]


def _assert_declared(obj):
    """No instance dictionary to grow, and every slot was assigned by the constructor."""
    assert not hasattr(obj, '__dict__'), type(obj).__name__
    names = _slots(obj)
    assert names, type(obj).__name__
    for s in names:
        getattr(obj, s)         # AttributeError: a slot that __init__ left unset


@pytest.mark.parametrize('reduce_scatter', [False, True])
def test_no_attribute_appears_after_construction(gloo_rank0, reduce_scatter):
    from exploremultimodal_amd import dp
    torch.manual_seed(0)
    model = Two()
    red = dp.GradReducer(model, reduce_scatter=reduce_scatter, engine_sink=False)
    try:
        before = set(vars(red).keys())
        assert [b.name for b in red.buckets] == ['block000', 'rest']
        for b in red.buckets:
            _assert_declared(b)
        # a sink bucket and an arena straight from their constructors
        fresh_arena = dp._Arena(64, torch.device('cpu'), torch.float32)
        _assert_declared(fresh_arena)
        _assert_declared(dp._SinkBucket(20, torch.device('cpu'), torch.float32, 1, fresh_arena))
        _assert_declared(dp._SinkBucket(20, torch.device('cpu'), torch.float32, 1))

        group = tuple(model.blocks[0].parameters())
        n = sum(p.numel() for p in group)
        for step, accumulate in enumerate([True, False]):
            x = torch.ones(3, 4, requires_grad=True)
            y = _FakeEngineFn.apply(x, red, [group], float(step + 1))      # expect() / acquire() / release_all()
            loss = model.head(y).sum()
            red.prepare(loss)
            loss.backward()
            red.finish(accumulate=accumulate)
            assert set(vars(red).keys()) == before, (step, set(vars(red).keys()) ^ before)

        # both kinds of bucket went through an exchange
        (sb,) = red.sinks.values()
        rest = red.buckets[1]
        assert sb.has_grad and rest.has_grad and rest.had == [True, True]
        assert sb.had is None, 'zero.ZeroAdam tells a sink bucket from a hook bucket by this'
        if reduce_scatter:
            assert sb.shard is sb.shard32 and rest.shard is rest.shard32
            assert torch.equal(sb.shard[:n], torch.full((n,), 3.0))         # 1 + 2 accumulated, world size 1
        else:
            assert torch.equal(sb.flat[:n], torch.full((n,), 3.0))
            assert model.head.weight.grad.data_ptr() == rest.flat.data_ptr()
        for b in list(red.buckets) + list(red.sinks.values()):
            _assert_declared(b)
    finally:
        red.close()


def test_no_defaulted_getattr_or_hasattr_in_dp_and_zero():
    from exploremultimodal_amd import dp, zero
    for mod in (dp, zero):
        with open(mod.__file__) as f:
            tree = ast.parse(f.read())
        bad = [(node.func.id, node.lineno) for node in ast.walk(tree)
               if isinstance(node, ast.Call) and isinstance(node.func, ast.Name)
               and (node.func.id == 'hasattr' or (node.func.id == 'getattr' and len(node.args) + len(node.keywords) >= 3))]
        assert not bad, (mod.__name__, bad)
