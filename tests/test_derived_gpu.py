"""The derived weights of the tokenizers and the vocabulary heads (derived.of) on the engine: after an in-place write to
a master weight the next call computes with the new value, bit for bit what a module built fresh from the state dict
computes.  Every case first runs once, so the derived tensors exist and can go stale."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda')

from exploremultimodal_amd import dvae, heads  # noqa: E402


def _twin(make, src):
    t = make()
    t.load_state_dict(src.state_dict(), strict=True)
    return t


def _write(params, seed):
    """In-place writes (version bumps) that change every entry."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in params:
            p.mul_(0.5).add_((torch.randn(p.shape, generator=g) * 0.05).to(p.device))


@pytest.fixture(scope='module')
def images():
    return torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(0)).to(DEV)


def _encoder():
    return dvae.Encoder(n_hid=256, vocab_size=512, device=DEV)


def test_encoder_output_bias_written_in_place_decides_the_ids(images):
    """A guard on the engine path, not the demonstration of the unkeyed bias: this bias is fp32, and an fp32 bias was
    cached as an alias of the parameter, so the write was seen before too.  The half-precision case that went stale is
    tests/test_derived_cpu.py::test_half_bias_is_part_of_the_key."""
    torch.manual_seed(1)
    enc = _encoder()
    first = enc.codebook_indices(images)
    assert first.shape == (2, 4, 4)
    j = 137
    assert not (first == j).all()
    with torch.no_grad():
        enc.blocks.output.conv.b[j] += 1e4
    assert (enc.codebook_indices(images) == j).all()
    assert (enc(images).argmax(1) == j).all()


def test_encoder_follows_a_zeroed_weight_like_a_fresh_twin(images):
    torch.manual_seed(2)
    enc = _encoder()
    logits0, ids0 = enc(images).clone(), enc.codebook_indices(images)
    with torch.no_grad():
        enc.blocks.group_1.block_1.res_path.conv_1.w.zero_()
    twin = _twin(_encoder, enc)
    logits, ids = enc(images), enc.codebook_indices(images)
    assert not torch.equal(logits, logits0)
    assert torch.equal(logits, twin(images)) and torch.equal(ids, twin.codebook_indices(images))
    # the fused tail [conv_4.w | id_path.w] and its combined bias follow each of their four tensors
    blk = enc.blocks.group_2.block_1
    _write([blk.res_path.conv_4.w, blk.res_path.conv_4.b, blk.id_path.w, blk.id_path.b], seed=3)
    twin = _twin(_encoder, enc)
    assert torch.equal(enc(images), twin(images))
    assert torch.equal(enc.codebook_indices(images), twin.codebook_indices(images))


def test_decoder_follows_in_place_writes_like_a_fresh_twin():
    torch.manual_seed(4)
    make = lambda: dvae.Decoder(n_hid=256, vocab_size=1024, device=DEV)
    dec = make()
    ids = torch.randint(0, 1024, (2, 4, 4), generator=torch.Generator().manual_seed(5)).to(DEV)
    out0 = dec.decode_ids(ids).clone()
    assert out0.shape == (2, 6, 32, 32)
    blk = dec.blocks.group_1.block_1
    _write([dec.blocks.input.w, dec.blocks.input.b, blk.id_path.w, blk.res_path.conv_4.b, dec.blocks.output.conv.w,
            dec.blocks.output.conv.b], seed=6)
    out = dec.decode_ids(ids)
    assert not torch.equal(out, out0)
    assert torch.equal(out, _twin(make, dec).decode_ids(ids))


def test_customized_tokenizer_follows_in_place_writes_like_a_fresh_twin(images):
    torch.manual_seed(7)
    make = lambda: dvae.DiscreteVAE(image_size=32, num_tokens=512, codebook_dim=64, num_layers=3, hidden_dim=64).to(DEV)
    vae = make()
    ids0 = vae.get_codebook_indices(images)
    seq = torch.randint(0, 512, (2, 16), generator=torch.Generator().manual_seed(8)).to(DEV)
    img0 = vae.decode(seq).clone()
    assert ids0.shape == (2, 4, 4) and img0.shape == (2, 3, 32, 32)
    head = vae.encoder[6]
    _write([vae.encoder[0][0].weight, vae.encoder[1].net[0].bias, vae.encoder[2][0].weight, head.weight, head.bias,
            vae.codebook.weight, vae.decoder[0][0].weight, vae.decoder[1].net[4].weight, vae.decoder[6].bias], seed=9)
    twin = _twin(make, vae)
    logits = vae(images, return_logits=True)
    assert torch.equal(logits, twin(images, return_logits=True))
    assert torch.equal(vae.get_codebook_indices(images), twin.get_codebook_indices(images))
    img = vae.decode(seq)
    assert not torch.equal(img, img0)
    assert torch.equal(img, twin.decode(seq))


def test_mim_head_follows_in_place_writes_like_a_fresh_twin():
    torch.manual_seed(10)
    make = lambda: heads.MIMHead(64, 128).to(DEV)
    head = make()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(8, 64, generator=g).to(DEV)
    labels = torch.randint(0, 128, (8,), generator=g)
    labels[3] = -100
    labels = labels.to(DEV)
    loss0, _ = head.loss_and_pred(x, labels)
    for p in (head.fc.weight, head.fc.bias):          # one at a time: each is in the key
        _write([p], seed=12)
        twin = _twin(make, head)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        loss, pred = head.loss_and_pred(xa, labels)
        tloss, tpred = twin.loss_and_pred(xb, labels)
        assert not torch.equal(loss, loss0)
        assert torch.equal(loss, tloss) and torch.equal(pred, tpred)
        loss.backward()
        tloss.backward()
        assert torch.equal(xa.grad, xb.grad) and torch.equal(head.fc.weight.grad, twin.fc.weight.grad)
        assert torch.equal(head.fc.bias.grad, twin.fc.bias.grad)
        head.zero_grad(set_to_none=True)
        loss0 = loss.detach()
