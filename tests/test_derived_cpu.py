"""derived.Holder / derived.of and what the dVAE and the heads keep in them: staleness keys, one slot per result, nothing
stored on (or travelling with) the owning module.  Host code only."""
import copy
import gc
import io
import os

import pytest
import torch

from exploremultimodal_amd import derived, dvae, heads

PKL = os.path.join(os.path.dirname(__file__), 'golden', 'dvae_encoder_pickle.pkl')


def _convs(m):
    return [c for c in m.modules() if isinstance(c, dvae.Conv2d)]


def _build_all(enc):
    """Every derived tensor the encoder's engine path reads."""
    for c in _convs(enc):
        c.shadow() if c.use_float16 else c.shadow_split()
    tails = [b for b in enc.modules() if isinstance(b, dvae.EncoderBlock) and isinstance(b.id_path, dvae.Conv2d)]
    assert tails
    for b in tails:
        b.tail_shadow()
    return tails


# ---------------------------------------------------------------- the primitive
def test_holder_rebuilds_per_tensor_in_the_key():
    h = derived.Holder()
    a, b = torch.zeros(4), torch.ones(3)
    calls = []

    def build():
        calls.append(1)
        return (a * 2, b.clone())
    first = h.get('s', (a, b, None), build)
    assert h.get('s', (a, b, None), build) is first and len(calls) == 1
    for t in (a, b):
        with torch.no_grad():
            t.add_(1.0)
        got = h.get('s', (a, b, None), build)
        assert got is not first
        first = got
        assert h.get('s', (a, b, None), build) is first
    assert len(calls) == 3
    assert h.get('s', (a, b, b), build) is not first          # None against a tensor
    assert h.get('other', (a,), lambda: 7) == 7 and set(h.slots) == {'s', 'other'}


def test_holder_key_carries_the_dtype():
    h = derived.Holder()
    t = torch.zeros(4)
    first = h.get('s', (t,), lambda: object())
    u = t.view(torch.int32)                                   # same version counter, same address
    assert (u._version, u.data_ptr()) == (t._version, t.data_ptr())
    assert h.get('s', (u,), lambda: object()) is not first


@pytest.mark.parametrize('method', ['shadow', 'shadow_split', 'shadow_embed'])
def test_conv_shadows_follow_writes_and_moves(method):
    c = dvae.Conv2d(64, 64, 1, use_float16=method == 'shadow')
    get = getattr(c, method)
    first = get()
    assert get() is first
    for p in (c.w, c.b):
        with torch.no_grad():
            p.add_(1.0)
        got = get()
        assert got is not first and get() is got
        first = got
    c.half()                                                  # new storage
    got = get()
    assert got is not first and torch.equal(got[1], c.b.float())
    c.to(torch.float64)
    assert get() is not got


def test_tail_shadow_follows_each_of_its_four_tensors():
    blk = dvae.EncoderBlock(64, 128, n_layers=8)
    c4, idp = blk.res_path.conv_4, blk.id_path
    first = blk.tail_shadow()
    assert blk.tail_shadow() is first
    for p in (c4.w, c4.b, idp.w, idp.b):
        with torch.no_grad():
            p.add_(0.5)
        got = blk.tail_shadow()
        assert got is not first and blk.tail_shadow() is got
        first = got
    w, b = first
    assert torch.equal(w, torch.cat([c4.shadow()[0], idp.shadow()[0]], 1))
    assert torch.equal(b, blk.post_gain * c4.b.detach() + idp.b.detach())
    blk.half()
    assert blk.tail_shadow() is not first


def test_conv_shadow_and_codebook_table_follow_writes():
    vae = dvae.DiscreteVAE(image_size=32, num_tokens=512, codebook_dim=64, num_layers=3, hidden_dim=64)
    conv = vae.encoder[1].net[0]
    first = dvae._conv_shadow(conv)
    assert dvae._conv_shadow(conv) is first
    for p in (conv.weight, conv.bias):
        with torch.no_grad():
            p.add_(1.0)
        got = dvae._conv_shadow(conv)
        assert got is not first
        first = got
    assert torch.equal(first[0], dvae.tap_major_shadow(conv.weight)) and torch.equal(first[1], conv.bias.detach())
    table = vae._codebook_table()
    assert vae._codebook_table() is table
    with torch.no_grad():
        vae.codebook.weight.add_(1.0)
    assert vae._codebook_table() is not table
    assert torch.equal(vae._codebook_table()[0][:, :64], vae.codebook.weight.detach())


# ---------------------------------------------------------------- the four faults
def test_half_bias_is_part_of_the_key():
    c = dvae.Conv2d(64, 64, 3).half()
    c.shadow()
    with torch.no_grad():
        c.b.add_(1.0)
    assert torch.equal(c.shadow()[1], c.b.float()) and c.shadow()[1].dtype == torch.float32
    o = dvae.Conv2d(64, 512, 1, use_float16=False).half()
    o.shadow_split()
    with torch.no_grad():
        o.b.add_(1.0)
    assert torch.equal(o.shadow_split()[1], o.b.float())


def test_shadow_and_shadow_split_do_not_evict_each_other():
    o = dvae.Conv2d(64, 512, 1, use_float16=False)
    a = o.shadow_split()
    s = o.shadow()
    assert o.shadow_split() is a and o.shadow_split()[0] is a[0]
    assert o.shadow() is s
    e = o.shadow_embed()
    assert o.shadow() is s and o.shadow_split() is a and o.shadow_embed() is e


def _saved(m):
    buf = io.BytesIO()
    torch.save(m, buf)
    return buf.getvalue()


def _stray_tensors(root):
    return [(n, k) for n, m in root.named_modules() for k, v in vars(m).items()
            if k not in ('_parameters', '_buffers') and
            any(isinstance(x, torch.Tensor) for x in (v if isinstance(v, (tuple, list)) else (v,)))]


def test_caches_do_not_travel_with_the_module():
    enc = dvae.Encoder(n_hid=64, vocab_size=512)
    before = _saved(enc)
    tails = _build_all(enc)
    assert _saved(enc) == before
    assert _stray_tensors(enc) == []
    twin = copy.deepcopy(enc)
    assert _stray_tensors(twin) == []
    for a, b in zip(_convs(enc) + tails, _convs(twin) + [m for m in twin.modules() if isinstance(m, dvae.EncoderBlock)
                                                         and isinstance(m.id_path, dvae.Conv2d)]):
        assert derived.of(a).slots and derived.of(b).slots == {} and derived.of(a) is not derived.of(b)
    # the copy builds its own, from its own tensors
    c0, t0 = _convs(enc)[0], _convs(twin)[0]
    assert t0.shadow()[0] is not c0.shadow()[0] and torch.equal(t0.shadow()[0], c0.shadow()[0])

    head = heads.MIMHead(64, 128)
    w, b = head.fc.weight, head.fc.bias
    built = derived.of(head).get('ce', (w, b), lambda: heads._pad_vocab_head(w, b))
    assert derived.of(head).get('ce', (w, b), lambda: heads._pad_vocab_head(w, b)) is built
    assert _stray_tensors(head) == [] and set(head.state_dict()) == {'fc.weight', 'fc.bias'}
    head2 = copy.deepcopy(head)
    assert derived.of(head2) is not derived.of(head) and derived.of(head2).slots == {}
    assert set(derived.of(head).slots) == {'ce'}


def test_loaded_pickle_needs_no_fix_up():
    enc = dvae.load_model(PKL, device='cpu')
    assert _convs(enc)
    for m in enc.modules():
        assert '_shadow' not in vars(m) and '_tail' not in vars(m) and '_embed' not in vars(m)


def test_holder_dies_with_its_owner():
    owner = dvae.Conv2d(64, 64, 1)
    gc.collect()
    owner.shadow()
    n = len(derived._holders)
    del owner
    gc.collect()
    assert len(derived._holders) == n - 1
