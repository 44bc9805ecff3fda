"""Weight average (ema.ModelEma), host logic: the update rule against the fp64 recurrence, the exact fixed point, the
timm ModelEmaV2 surface, and the 'model_ema' entry of the checkpoint format (utils/utils.py:486-508, 537-623).

Bound of the float comparisons: one update e + w (p - e) rounds three times at most (the difference, the product, the
sum; a fused multiply-add saves one), each by at most 2^-24 relative to a value no larger than max(|e|, |p|) -- the
result lies between e and p, the product is smaller than the difference.  An error already in e is carried with
factor 1 - w < 1, so over S updates the bound is 3 S 2^-24 max(|e|, |p|), the maximum taken over the S steps."""
import copy

import pytest
import torch

from exploremultimodal_amd import checkpoint, optim
from exploremultimodal_amd.build import build_model
from oracle import synth


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(13, 7)
        self.norm = torch.nn.LayerNorm(7)
        self.frozen = torch.nn.Parameter(torch.randn(5, 3), requires_grad=False)
        self.register_buffer('running', torch.randn(7))
        self.register_buffer('count', torch.zeros((), dtype=torch.int64))


def _ema():
    from exploremultimodal_amd.ema import ModelEma
    return ModelEma


@pytest.mark.parametrize('decay', [0.9, 0.9999])
def test_update_follows_the_fp64_recurrence(decay):
    ModelEma = _ema()
    torch.manual_seed(0)
    net = _Net().train()
    ema = ModelEma(net, decay=decay)
    w = 1.0 - decay
    ref = {k: v.double().clone() for k, v in net.state_dict().items()}
    big = {k: v.abs().double() for k, v in net.state_dict().items()}
    steps = 20
    for s in range(steps):
        with torch.no_grad():
            for k, v in net.state_dict().items():
                if k == 'frozen':
                    continue
                if v.is_floating_point():
                    v.add_(torch.randn_like(v) * 0.3)
                else:
                    v.add_(s + 1)
        ema.update(net)
        for k, p in net.state_dict().items():
            if p.is_floating_point():
                ref[k] = ref[k] + w * (p.double() - ref[k])
                big[k] = torch.maximum(big[k], torch.maximum(ref[k].abs(), p.abs().double()))
    got = ema.state_dict()
    assert list(got) == list(net.state_dict())
    for k, p in net.state_dict().items():
        if p.is_floating_point():
            err = (got[k].double() - ref[k].float().double()).abs()
            bound = 3 * steps * 2.0 ** -24 * big[k]
            assert (err <= bound).all(), (k, err.max().item(), bound.min().item())
            if k != 'frozen':
                assert not torch.equal(got[k], p), k          # an average, not a copy
        else:
            assert got[k].dtype == torch.int64 and torch.equal(got[k], p), k


def test_an_unchanged_source_is_an_exact_fixed_point():
    ModelEma = _ema()
    torch.manual_seed(1)
    net = _Net()
    ema = ModelEma(net, decay=0.9999)
    start = copy.deepcopy(ema.state_dict())
    for _ in range(1000):
        ema.update(net)
    for k, v in ema.state_dict().items():
        assert torch.equal(v, start[k]) and torch.equal(v, net.state_dict()[k]), k


def test_surface_set_and_refusals():
    ModelEma = _ema()
    torch.manual_seed(2)
    net = _Net().train()
    ema = ModelEma(net, decay=0.5)
    assert not ema.module.training and net.training
    assert not any(p.requires_grad for p in ema.module.parameters())
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(ema.state_dict().values(), net.state_dict().values()))
    with torch.no_grad():
        net.fc.weight.add_(1.0)
        net.count.add_(3)
    assert not torch.equal(ema.module.fc.weight, net.fc.weight)
    v0 = ema.module.fc.weight._version
    ema.set(net)
    assert ema.module.fc.weight._version > v0
    for k, v in ema.state_dict().items():
        assert torch.equal(v, net.state_dict()[k]), k
    # the decay is read at every update
    with torch.no_grad():
        net.fc.bias.add_(2.0)
    ema.decay = 0.0
    v0 = ema.module.fc.bias._version
    ema.update(net)
    assert torch.equal(ema.module.fc.bias, net.fc.bias)
    assert ema.module.fc.bias._version > v0                  # version counters move: cached weight copies refresh
    ema.decay = 1.0
    held = ema.module.fc.bias.detach().clone()
    with torch.no_grad():
        net.fc.bias.add_(2.0)
    ema.update(net)
    assert torch.equal(ema.module.fc.bias, held)
    # state dict round trip of .module
    other = ModelEma(_Net(), decay=0.5)
    other.load_state_dict(ema.state_dict())
    for k, v in other.state_dict().items():
        assert torch.equal(v, ema.state_dict()[k]), k
    # mismatches are refused by name
    wider = _Net()
    wider.fc = torch.nn.Linear(13, 8)
    with pytest.raises(ValueError, match='fc.weight'):
        ema.update(wider)
    extra = _Net()
    extra.register_buffer('surplus', torch.zeros(2))
    with pytest.raises(KeyError, match='surplus'):
        ema.update(extra)
    ema.decay = 1.5
    with pytest.raises(ValueError, match='decay'):
        ema.update(net)


def test_tied_weights_are_averaged_once_per_update():
    ModelEma = _ema()
    net = torch.nn.Module()
    net.a = torch.nn.Linear(4, 4, bias=False)
    net.b = torch.nn.Linear(4, 4, bias=False)
    net.b.weight = net.a.weight
    ema = ModelEma(net, decay=0.5)
    assert ema.module.a.weight is ema.module.b.weight
    e0 = ema.module.a.weight.detach().clone()
    with torch.no_grad():
        net.a.weight.add_(1.0)
    ema.update(net)
    torch.testing.assert_close(ema.module.a.weight, e0 + 0.5, rtol=0, atol=1e-6)      # once, not 0.75 of the way


def _cfg(tmp, **over):
    cfg = synth.make_config('mini', loss_names=['mlm', 'itc'], **over)
    cfg.train.auto_resume, cfg.train.resume, cfg.train.epochs, cfg.train.start_epoch = True, '', 10, 0
    cfg.tag, cfg.exp_dir, cfg.output_dir = 'unit', str(tmp), str(tmp / 'run0')
    return cfg


class _Sched:
    def state_dict(self):
        return {}

    def load_state_dict(self, sd):
        pass


def test_checkpoint_round_trip_of_the_average(tmp_path):
    ModelEma = _ema()
    cfg = _cfg(tmp_path)
    torch.manual_seed(0)
    model = build_model(cfg)
    ema = ModelEma(model, decay=0.9)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.randn_like(p) * 0.01)
    ema.update(model)
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    scaler = optim.NativeScalerWithGradNormCount()
    name = checkpoint.save_model(cfg, 1, model, model, opt, _Sched(), scaler, model_ema=ema)
    raw = torch.load(tmp_path / 'run0' / name, weights_only=False)
    assert list(raw['model_ema']) == list(raw['model'])
    assert any(not torch.equal(raw['model_ema'][k], raw['model'][k]) for k in raw['model'])

    def fresh(seed):
        cfg2 = _cfg(tmp_path)
        torch.manual_seed(seed)
        m = build_model(cfg2)
        return cfg2, m, ModelEma(m, decay=0.9), torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3)

    cfg2, model2, ema2, opt2 = fresh(1)
    checkpoint.auto_load_model(cfg2, model2, model2, opt2, _Sched(), scaler, model_ema=ema2)
    assert cfg2.train.start_epoch == 2
    for k, v in ema2.state_dict().items():
        assert torch.equal(v, ema.state_dict()[k]), k
        assert torch.equal(model2.state_dict()[k], model.state_dict()[k]), k
    # a checkpoint without the entry: the average restarts from the loaded weights
    checkpoint.save_model(cfg, 2, model, model, opt, _Sched(), scaler)
    cfg3, model3, ema3, opt3 = fresh(2)
    checkpoint.auto_load_model(cfg3, model3, model3, opt3, _Sched(), scaler, model_ema=ema3)
    assert cfg3.train.resume.endswith('checkpoint-2.pth')
    for k, v in ema3.state_dict().items():
        assert torch.equal(v, model.state_dict()[k]), k
        assert v.data_ptr() != model3.state_dict()[k].data_ptr()


def test_the_momentum_twin_stays_refused(tmp_path):
    cfg = _cfg(tmp_path)
    cfg.vlmo_ema = True
    with pytest.raises(NotImplementedError, match='vlmo_ema'):
        build_model(cfg)
