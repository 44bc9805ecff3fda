"""exploremultimodal_amd.retrieval without a GPU: recall_at_k against a plain Python loop, the ordering rule of the CPU
sim_topk (the yardstick of the HIP kernel's tests), and planted data with a known recall."""
import pytest
import torch

from exploremultimodal_amd import retrieval as R


def _recall_loop(indices, txt2img, direction, ks):
    out = []
    for k in ks:
        hits = 0
        for qi, row in enumerate(indices.tolist()):
            first = [e for e in row[:k] if e >= 0]
            if direction == 't2i':
                hits += int(txt2img[qi].item() in first)
            else:
                hits += int(any(txt2img[c].item() == qi for c in first))
        out.append(hits / indices.shape[0])
    return out


def _unit(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float()


def test_recall_matches_python_loop_both_directions():
    g = torch.Generator().manual_seed(3)
    n_img = 9
    # image 0: 3 captions, image 1: 1, image 4: none (nor 7, 8), the others 2 or 5
    txt2img = torch.tensor([0, 0, 0, 1, 2, 2, 3, 3, 5, 5, 5, 5, 5, 6, 6])
    n_txt = txt2img.numel()
    ks = (1, 3, 10)                                       # image 1 has one positive: k = 10 is far beyond it
    t2i = torch.stack([torch.randperm(n_img, generator=g) for _ in range(n_txt)])
    t2i = torch.cat([t2i, torch.full((n_txt, 1), -1)], 1)                 # Ng = 9 < K = 10: the fill of sim_topk
    i2t = torch.stack([torch.randperm(n_txt, generator=g)[:10] for _ in range(n_img)])
    i2t[2, 0] = -1
    i2t[4, :] = -1                                        # -1 must never read txt2img[-1]
    i2t[6, 3:] = -1
    for ind, d in ((t2i, 't2i'), (i2t, 'i2t')):
        got = R.recall_at_k(ind, txt2img, d, ks)
        assert got.dtype == torch.float32 and got.shape == (3,)
        assert got.tolist() == pytest.approx(_recall_loop(ind, txt2img, d, ks), abs=1e-6)
        assert 0.0 <= got.min() and got.max() <= 1.0
    # the caption of the last image slot: an index of -1 is not "caption n_txt - 1"
    only_fill = torch.full((n_img, 1), -1)
    assert R.recall_at_k(only_fill, txt2img, 'i2t', (1,)).item() == 0.0
    with pytest.raises(ValueError):
        R.recall_at_k(i2t, txt2img, 'i2t', (11,))
    with pytest.raises(ValueError):
        R.recall_at_k(i2t, txt2img, 'both', (1,))


def test_cpu_topk_duplicates_come_in_index_order():
    g = _unit(40, 32, 5)
    g[7] = g[31]
    g[12] = g[31]
    g[3] = g[20]
    q = torch.cat([g[31:32], g[20:21], _unit(4, 32, 6)])
    val, idx = R.sim_topk(q, g, 5)
    assert idx.dtype == torch.int64 and val.dtype == torch.float32
    assert idx[0, :3].tolist() == [7, 12, 31] and val[0, 0] == val[0, 1] == val[0, 2]
    assert idx[1, :2].tolist() == [3, 20]
    assert (val[:, :-1] >= val[:, 1:]).all()
    # all-equal scores: pure index order
    val, idx = R.sim_topk(torch.ones(2, 8), torch.ones(20, 8), 16, scale=0.5)
    assert idx.tolist() == [list(range(16))] * 2 and (val == 4.0).all()


def test_cpu_topk_short_gallery_is_filled():
    q, g = _unit(3, 16, 1), _unit(5, 16, 2)
    val, idx = R.sim_topk(q, g, 10)
    assert val.shape == idx.shape == (3, 10)
    assert (idx[:, 5:] == -1).all() and torch.isinf(val[:, 5:]).all() and (val[:, 5:] < 0).all()
    assert sorted(idx[0, :5].tolist()) == [0, 1, 2, 3, 4]
    ref = (q.double() @ g.double().t()).float()
    assert torch.equal(val[:, :5], ref.sort(1, descending=True).values)


def test_cpu_topk_does_not_depend_on_the_chunk_size():
    q, g = _unit(37, 64, 11), _unit(129, 64, 12)
    g[100] = g[4]
    base = R._sim_topk_cpu(q, g, 10, 2.0)
    for rows in (1, 5, 36, 37, 1000):
        val, idx = R._sim_topk_cpu(q, g, 10, 2.0, chunk_rows=rows)
        assert torch.equal(idx, base[1]) and torch.equal(val, base[0]), rows
    # the public entry's own slab height
    val, idx = R.sim_topk(q, g, 10, scale=2.0)
    assert torch.equal(idx, base[1]) and torch.equal(val, base[0])


def test_cpu_topk_refuses_what_the_kernel_refuses():
    q, g = _unit(3, 16, 1), _unit(5, 16, 2)
    for bad in (dict(k=17), dict(k=0), dict(k=3, scale=0.0)):
        with pytest.raises(ValueError):
            R.sim_topk(q, g, **bad)
    with pytest.raises(ValueError):
        R.sim_topk(q[:, :6], g[:, :6], 3)                 # D % 4 != 0
    with pytest.raises(ValueError):
        R.sim_topk(q.half(), g.half(), 3)
    with pytest.raises(ValueError):
        R.sim_topk(q, _unit(5, 20, 2), 3)


def test_planted_captions_give_recall_one():
    n_img, per = 40, 3
    img = _unit(n_img, 64, 21)
    txt2img = torch.arange(n_img).repeat_interleave(per)
    noise = 0.02 * torch.randn(n_img * per, 64, generator=torch.Generator().manual_seed(22))
    txt = torch.nn.functional.normalize(img[txt2img] + noise, dim=1)
    out = R.recall_from_features(img, txt, txt2img)
    assert set(out) == {'ir_r1', 'ir_r5', 'ir_r10', 'tr_r1', 'tr_r5', 'tr_r10', 'r_mean'}
    assert all(v == 1.0 for v in out.values()), out
    assert all(isinstance(v, float) for v in out.values())


def test_known_permutation_gives_the_recall_computed_by_hand():
    """10 orthogonal images, one caption each.  Captions 0-5 sit on their image; 6 and 7 are closest to a wrong image
    with their own second; 8 and 9 have their own image third.  t2i: R@1 = 6/10, R@2 = 8/10, R@3 = 1.  The captions
    are nearly one-hot, so i2t: image i ranks caption i first unless another caption leans on it harder: images 0..5
    and 6..9 all see their own caption with weight >= 0.8 against <= 0.5 from the others -> R@1 = 1."""
    n = 10
    img = torch.eye(n, 16)
    txt = torch.zeros(n, 16)
    for t in range(6):
        txt[t, t] = 1.0
    for t in (6, 7):
        txt[t, t] = 0.8
        txt[t, t - 6] = 0.9          # wrong image first, own second
    for t in (8, 9):
        txt[t, t] = 0.8
        txt[t, t - 8] = 0.95
        txt[t, t - 6] = 0.9          # own image third
    txt2img = torch.arange(n)
    _, t2i = R.sim_topk(txt, img, 3)
    assert R.recall_at_k(t2i, txt2img, 't2i', (1, 2, 3)).tolist() == pytest.approx([0.6, 0.8, 1.0])
    # image-to-text: image 0 sees captions 0 (1.0), 8 (0.95), 6 (0.9); image 2 sees 2 (1.0), 8 (0.9); image 6 sees 6 (0.8)
    _, i2t = R.sim_topk(img, txt, 3)
    assert i2t[0].tolist() == [0, 8, 6] and i2t[2, :2].tolist() == [2, 8] and i2t[6, 0].item() == 6
    assert R.recall_at_k(i2t, txt2img, 'i2t', (1, 2, 3)).tolist() == pytest.approx([1.0, 1.0, 1.0])
    out = R.recall_from_features(img, txt, txt2img, ks=(1, 2, 3))
    assert out['ir_r1'] == pytest.approx(0.6) and out['ir_r2'] == pytest.approx(0.8) and out['tr_r1'] == 1.0
    assert out['r_mean'] == pytest.approx((0.6 + 0.8 + 1.0 + 3.0) / 6)


def test_encode_refuses_a_model_without_itc_head():
    with pytest.raises(ValueError, match='itc'):
        R.encode_images(torch.nn.Linear(2, 2), torch.zeros(1, 3, 8, 8))
