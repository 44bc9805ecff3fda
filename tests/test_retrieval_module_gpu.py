"""exploremultimodal_amd.retrieval on the mini synthetic model with loss_names = ['itc']: 12 images, 36 captions (three
per image).  Tensor tolerance: atol 1e-6, the one tests/test_module_gpu.py holds the module's outputs to when the same
rows pass through differently composed batches (rows are independent: LayerNorm per token, attention per sequence)."""
import pytest
import torch

from exploremultimodal_amd import retrieval as R
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
N_IMG, PER = 12, 3
ATOL = 1e-6


@pytest.fixture(scope='module')
def setup():
    from exploremultimodal_amd.build import build_model
    cfg = synth.make_config('mini', loss_names=['itc'])
    model = build_model(cfg)
    sd = {'transformer.' + k: v for k, v in synth.synth_backbone_state_dict(cfg.model, 0).items()}
    sd.update(synth.synth_head_state_dict(cfg.model, 0, ['itc']))
    r = model.load_state_dict(sd, strict=False)
    assert not r.unexpected_keys and not r.missing_keys, r
    model = model.to(DEV).eval()
    images = synth.synth_batch(cfg.model, N_IMG, seed=31, mim=False)['image'].to(DEV)
    tb = synth.synth_batch(cfg.model, N_IMG * PER, seed=32, mim=False)
    txt2img = torch.arange(N_IMG).repeat_interleave(PER)
    return model, images, tb['text_ids'].to(DEV), tb['text_mask'].to(DEV), txt2img.to(DEV)


def test_encode_equals_infer_plus_itc_head(setup):
    model, images, ids, mask, _ = setup
    with torch.no_grad():
        i_ref = model.itc_head(model.infer({'image': images}, infer_mode='img_only')['co_feats'][:, 0], 'v')
        t_ref = model.itc_head(model.infer({'text_ids': ids, 'text_mask': mask}, infer_mode='txt_only')['co_feats'][:, 0], 'l')
    i_feat = R.encode_images(model, images, batch_size=12)
    t_feat = R.encode_texts(model, ids, mask, batch_size=36)
    itc_dim = model.config.model.itc_dim
    assert i_feat.shape == (N_IMG, itc_dim) and t_feat.shape == (N_IMG * PER, itc_dim)
    assert i_feat.dtype == t_feat.dtype == torch.float32 and not i_feat.requires_grad
    for got, ref in ((i_feat, i_ref), (t_feat, t_ref)):
        err = (got - ref).abs().max().item()
        print('max |encode - direct| =', err)
        assert err <= ATOL
        assert (got.norm(dim=1) - 1).abs().max().item() <= 1e-6          # unit rows, to fp32 rounding


def test_encode_does_not_depend_on_the_batch_size(setup):
    model, images, ids, mask, _ = setup
    for a, b in ((R.encode_images(model, images, batch_size=5), R.encode_images(model, images, batch_size=12)),
                 (R.encode_texts(model, ids, mask, batch_size=5), R.encode_texts(model, ids, mask, batch_size=12))):
        err = (a - b).abs().max().item()
        print('max |batch 5 - batch 12| =', err)
        assert a.shape == b.shape and err <= ATOL


def test_training_flag_is_restored(setup):
    model, images, ids, mask, _ = setup
    try:
        model.train()
        out = R.encode_images(model, images[:3])
        assert model.training and not out.requires_grad
        R.encode_texts(model, ids[:3], mask[:3])
        assert model.training
        model.eval()
        R.encode_images(model, images[:3])
        assert not model.training
    finally:
        model.eval()


def test_evaluate_on_gpu_equals_cpu_path_on_the_same_features(setup):
    model, images, ids, mask, txt2img = setup
    got = R.evaluate_retrieval(model, images, ids, mask, txt2img, image_batch_size=5, text_batch_size=7)
    assert set(got) == {'ir_r1', 'ir_r5', 'ir_r10', 'tr_r1', 'tr_r5', 'tr_r10', 'r_mean'}
    i_feat = R.encode_images(model, images, batch_size=5).cpu()
    t_feat = R.encode_texts(model, ids, mask, batch_size=7).cpu()
    ref = R.recall_from_features(i_feat, t_feat, txt2img.cpu())
    print(got)
    for k in ref:
        assert got[k] == pytest.approx(ref[k], abs=1e-7), k
        assert 0.0 <= got[k] <= 1.0
    assert got['ir_r1'] <= got['ir_r5'] <= got['ir_r10'] and got['tr_r1'] <= got['tr_r5'] <= got['tr_r10']
    # the rankings themselves, where the CPU scores are not within rounding of each other
    for qf, gf in ((t_feat, i_feat), (i_feat, t_feat)):
        vg, ig = R.sim_topk(qf.to(DEV), gf.to(DEV), 10)
        vc, ic = R.sim_topk(qf, gf, 11)                  # one more: the gap below the last returned entry counts too
        bound = 32 * 2.0 ** -24 / (1 - 32 * 2.0 ** -24)  # itc_dim = 32
        assert (vg.cpu() - vc[:, :10]).abs().max().item() <= bound
        clear = (vc[:, :-1] - vc[:, 1:] > 4 * bound).all(1)
        assert torch.equal(ig.cpu()[clear], ic[clear, :10])


def test_model_without_itc_head_is_refused(setup):
    from exploremultimodal_amd.build import build_model
    model = build_model(synth.make_config('mini', loss_names=[]))
    with pytest.raises(ValueError, match='itc'):
        R.encode_images(model, setup[1])
    with pytest.raises(ValueError, match='itc'):
        R.evaluate_retrieval(model, *setup[1:])
