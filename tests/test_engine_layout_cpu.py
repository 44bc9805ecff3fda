"""Host logic of the engine that needs no GPU: the flat gradient-bucket layout that engine._fill_grads carves for
vlmo_stack_bwd must be the layout engine.group_layout advertises to the ZeRO-2 optimizer
(zero.ZeroAdam re-homes the parameters by these offsets), including the hole the zero k-bias leaves."""
import types

import pytest

import torch

from exploremultimodal_amd import engine


def test_bucket_layouts_match_the_carved_gradients():
    d, hid, nexp = 8, 32, 2
    mk = lambda *shape: torch.nn.Parameter(torch.zeros(*shape))
    shared = (mk(d), mk(d), mk(d), mk(d), mk(3 * d, d), mk(d), mk(d), mk(d, d), mk(d), mk(d), mk(d))
    experts = [(mk(hid, d), mk(hid), mk(d, hid), mk(d)) for _ in range(nexp)]
    shared_n = 6 * d + 3 * d * d + d * d + d + 3 * d
    exp_n = 2 * hid * d + hid + d
    flats = [torch.arange(shared_n, dtype=torch.float32)] + \
            [torch.arange(exp_n, dtype=torch.float32) + 1000 * (e + 1) for e in range(nexp)]

    class Desc:                 # stands in for the ctypes descriptor: accepts attribute and indexed writes
        def __init__(self):
            for n in ('dw1', 'db1', 'dw2', 'db2'):
                object.__setattr__(self, n, [0, 0])
    grads = engine._fill_grads(Desc(), flats, d, hid, nexp)
    assert len(grads) == 11 + 4 * nexp
    groups = engine.block_groups(list(shared) + [p for e in experts for p in e])
    shared_layout = engine.group_layout(groups[0], d, hid)
    for (p, off), g in zip(sorted(shared_layout, key=lambda t: [id(x) for x in shared].index(id(t[0]))),
                           grads[:11]):
        assert g.shape == p.shape
        assert g.reshape(-1)[0].item() == float(off), (p.shape, off)          # flat holds arange: first element = offset
        assert g.numel() == p.numel()
    for e in range(nexp):
        for (p, off), g in zip(engine.group_layout(groups[1 + e], d, hid), grads[11 + 4 * e: 15 + 4 * e]):
            assert g.shape == p.shape and g.reshape(-1)[0].item() == 1000.0 * (e + 1) + off
    # q_bias and v_bias sit at the two ends of the 3d-wide qkv-bias slot: the d elements between them have no parameter
    lay = dict((id(p), off) for p, off in shared_layout)
    assert lay[id(shared[6])] - lay[id(shared[5])] == 2 * d
    covered = sum(p.numel() for p in shared)
    assert shared_n - covered == d


def test_wgrad_batch_by_tile_count(monkeypatch):
    """engine.wgrad_batch_for: default two blocks per launch; VLMO_WGRAD_BATCH=0 = the count whose tiles fill whole rounds."""
    from exploremultimodal_amd import engine
    assert engine.wgrad_batch_for(768, 3072) == engine.WGRAD_BATCH == 2
    monkeypatch.setattr(engine, 'WGRAD_BATCH', 0)
    assert engine.wgrad_batch_for(768, 3072) == 2        # 108 tiles per block: 216 = one round of 256 CUs
    assert engine.wgrad_batch_for(1024, 4096) == 4       # 192 per block: 768 = exactly three rounds


def test_weight_gradient_stream_rule(monkeypatch):
    """engine._use_side_stream: forced by VLMO_OVERLAP_WGRAD (engine.OVERLAP_WGRAD True / False), else the side stream
    under a gradient reducer and for passes of fewer than ONE_STREAM_ROWS rows, the caller's stream otherwise."""
    sink = object()
    monkeypatch.setattr(engine, 'OVERLAP_WGRAD', None)
    assert engine._use_side_stream(None, 64 * 261) is False          # VLMo-Base at 64 pairs: one stream
    assert engine._use_side_stream(None, 32 * 261) is True           # VLMo-Large at 32 pairs: 8 352 rows
    assert engine._use_side_stream(None, engine.ONE_STREAM_ROWS) is False
    assert engine._use_side_stream(sink, 64 * 261) is True           # a reducer waits on per-block grad_ready events
    monkeypatch.setattr(engine, 'OVERLAP_WGRAD', False)
    assert engine._use_side_stream(sink, 100) is False
    monkeypatch.setattr(engine, 'OVERLAP_WGRAD', True)
    assert engine._use_side_stream(None, 1 << 20) is True


def test_dvae_output_convolution_row_parts(monkeypatch):
    """dvae.Encoder._row_parts: the rows of a last dispatch round of 256 x 256 tiles that is at most a quarter full go
    out as a second launch of 128 x 128 tiles; everything else stays one launch with the library's own tile choice."""
    from exploremultimodal_amd import dvae
    rp = dvae.Encoder._row_parts
    monkeypatch.setattr(dvae, 'OUTPUT_ROW_SPLIT', True)
    assert rp(64 * 196, 8192) == [(0, 12288, 3), (12288, 12544, 0)]          # 1 568 tiles = 6 rounds + 32
    assert rp(32 * 196, 8192) == [(0, 6144, 3), (6144, 6272, 0)]
    assert rp(2 * 196, 8192) == [(0, 392, -1)]                               # less than one round
    assert rp(8 * 256, 8192) == [(0, 2048, -1)]                              # exactly one round
    assert rp(8 * 256 + 3 * 256, 8192) == [(0, 2816, -1)]                    # last round 96 of 256 tiles: kept
    for M, N in ((12544, 8192), (6272, 8192), (5000, 2048), (70000, 512)):
        parts = rp(M, N)
        assert parts[0][0] == 0 and parts[-1][1] == M
        assert all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
        if len(parts) == 2:
            r = parts[0][1]
            assert r % 256 == 0 and (r // 256) * -(-N // 256) % 256 == 0     # the big launch fills whole rounds
    monkeypatch.setattr(dvae, 'OUTPUT_ROW_SPLIT', False)
    assert rp(64 * 196, 8192) == [(0, 12544, -1)]


# ---- the buffer layouts behind the descriptor pointers (engine.SLAB_BF16 / SLAB_F32 / TEMPS_BF16 / *_GRADS) --------------
# Every number below is written out here; none is obtained from the code under test.
M_ROWS = 261 * 2
FOUR_D = [(768, 3072), (1024, 4096), (128, 512)]
SLAB_COLS = lambda d, hid: dict(y1=d, qkv=3 * d, ctx=d, zd1=d, y2=d, u=hid, h=hid, zd2=d)
TEMP_COLS = lambda d, hid: dict(dz2=d, du=hid, dy2=d, dctx=d, dz1=d, dqkv=3 * d, dy1=d)


class _Desc:
    """Stands in for the ctypes descriptor: accepts attribute writes, and indexed writes to its array fields."""

    def __init__(self):
        for n in ('seg', 'nseq', 'maxlen', 'lse_stride', 'lse', 'attn_seed_idx', 'attn_seq0'):
            object.__setattr__(self, n, [None, None])


def _wire_slabs(d, hid, heads=2, pb=1 << 20, pf=1 << 30):
    D = _Desc()
    seg = [torch.zeros(4, 4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32)]
    engine._wire_slabs(D, pb, pf, M_ROWS, d, hid, heads, [(seg[0], 4, 261), (seg[1], 2, 64)])
    return D, seg


def _wire_temps(d, hid, k, nb=3, nsets=2, units=11):
    M = M_ROWS
    sc = engine._Scratch(nsets, 1, torch.empty(nsets * units * M * d, dtype=torch.bfloat16), torch.empty(2 * 6), 6,
                         torch.empty(3 * M * d))
    dxo, dx_in = torch.empty(1), torch.empty(1)
    D = _Desc()
    engine._wire_temporaries(D, k, nb, M, d, hid, sc, dxo, dx_in)
    return D, sc, dxo, dx_in


@pytest.mark.parametrize('d,hid', FOUR_D)
def test_wired_offsets_at_hidden_4d_are_frozen(d, hid):
    M, heads, pb, pf = M_ROWS, 2, 1 << 20, 1 << 30
    unit = M * d * 2                                        # bytes of M * d bf16 elements
    D, seg = _wire_slabs(d, hid, heads, pb, pf)
    assert {f: (getattr(D, f) - pb) / unit for f in SLAB_COLS(d, hid)} == \
        dict(y1=0, qkv=1, ctx=4, zd1=5, y2=6, u=7, h=11, zd2=15)
    L = engine._layouts(d, hid)
    assert L.slab.cols * M == 16 * M * d                    # the stride from one block's slab to the next
    SB = torch.empty(2 * 16 * M * d, dtype=torch.bfloat16)
    qkv = L.slab.view(SB, 1, M, 'qkv')
    assert qkv.shape == (M, 3 * d) and qkv.data_ptr() - SB.data_ptr() == (16 + 1) * unit and qkv.is_contiguous()
    # fp32 slab: x1, the four per-row statistics, then the log-sum-exp rows of the launches (stride ceil32(maxlen))
    assert D.x1 == pf
    assert [(p - pf) // 4 for p in (D.mean1, D.rstd1, D.mean2, D.rstd2)] == [M * d, M * d + M, M * d + 2 * M, M * d + 3 * M]
    assert (D.lse[0] - pf) // 4 == M * d + 4 * M
    assert D.lse_stride == [288, 64] and (D.lse[1] - D.lse[0]) // 4 == 4 * heads * 288
    assert L.f32.cols * M == M * d + 4 * M
    assert engine._lse_layout([(None, 4, 261), (None, 2, 64)], heads) == [(288, 4 * heads * 288), (64, 2 * heads * 64)]
    assert D.n_attn == 2 and D.nseq == [4, 2] and D.maxlen == [261, 64] and D.seg == [s.data_ptr() for s in seg]
    assert D.attn_seed_idx == [0, 1] and D.attn_seq0 == [0, 0]
    # the rotating temporaries: set k % nsets, 11 units apart; dctx shares dy2
    for k in range(3):
        D, sc, dxo, dx_in = _wire_temps(d, hid, k)
        base = sc.tb.data_ptr() + (k % 2) * 11 * unit
        assert {f: (getattr(D, f) - base) / unit for f in TEMP_COLS(d, hid)} == \
            dict(dz2=0, du=1, dy2=5, dctx=5, dz1=6, dqkv=7, dy1=10)
        assert D.ws_main == sc.ws.data_ptr() + (k % 2) * 6 * 4 and D.ws_bytes == 6 * 4
        assert D.dx1 == sc.dxs.data_ptr() + 2 * M * d * 4
        assert D.dx2 == (dxo.data_ptr() if k == 0 else sc.dxs.data_ptr() + ((k - 1) % 2) * M * d * 4)
        assert D.dx0 == (dx_in.data_ptr() if k == 2 else sc.dxs.data_ptr() + (k % 2) * M * d * 4)
        dctx = L.temps.view(sc.tb, k % 2, M, 'dctx')
        assert dctx.shape == (M, d) and dctx.data_ptr() == D.dctx == D.dy2
    assert L.temps.cols * M == 11 * M * d
    # gradient buckets
    blk = engine.block_groups([torch.zeros(1)] * (11 + 4))                     # group_numel reads the group kind only
    assert engine.group_numel(blk[0], d, hid) == 6 * d + 4 * d * d + 4 * d
    assert engine.group_numel(blk[1], d, hid) == 2 * hid * d + hid + d
    assert L.buckets[0].vectors == ((0, 6 * d), (6 * d + 4 * d * d, 6 * d + 4 * d * d + 4 * d))
    assert L.buckets[1].vectors == ((hid * d, hid * d + hid), (2 * hid * d + hid, 2 * hid * d + hid + d))


def _disjoint_inside(D, cols, base, nbytes, alias=()):
    rng = {f: (getattr(D, f), getattr(D, f) + M_ROWS * c * 2) for f, c in cols.items()}
    for f, (lo, hi) in rng.items():
        assert base <= lo < hi <= base + nbytes, f
    names = sorted(rng)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            if (a, b) in alias or (b, a) in alias:
                assert rng[a] == rng[b]
            else:
                assert rng[a][1] <= rng[b][0] or rng[b][1] <= rng[a][0], (a, b, rng[a], rng[b])


@pytest.mark.parametrize('ratio', [2, 3, 6])
def test_buffers_do_not_overlap_at_other_ffn_widths(ratio):
    """u, h and du are [M, hidden] matrices.  With the offsets that were literals (u at 7, h at 11, zd2 at 15 units of
    M * d, 16 to a slab; du at 1, dy2 at 5) this check fails at hidden = 6 d: u covers units [7, 13) and runs into h, h
    covers [11, 17) and ends one unit behind its block's 16-unit slab, du covers [1, 7) and runs into dy2.  That was
    the defect: nothing required hidden == 4 d."""
    d = 128
    hid, M = ratio * d, M_ROWS
    pb = 1 << 20
    D, _ = _wire_slabs(d, hid, pb=pb)
    cols = SLAB_COLS(d, hid)
    nbytes = engine._layouts(d, hid).slab.cols * M * 2
    assert nbytes == sum(cols.values()) * M * 2 == (8 * d + 2 * hid) * M * 2       # exactly as large as the matrices
    _disjoint_inside(D, cols, pb, nbytes)
    units = 7 + ratio
    for k in range(2):
        D, sc, _, _ = _wire_temps(d, hid, k, units=units)
        tcols = TEMP_COLS(d, hid)
        nbytes = engine._layouts(d, hid).temps.cols * M * 2
        assert nbytes == (7 * d + hid) * M * 2 == units * M * d * 2
        _disjoint_inside(D, tcols, sc.tb.data_ptr() + k * nbytes, nbytes, alias=[('dctx', 'dy2')])
    # every sub-buffer keeps the 128-byte alignment of its base (d and hidden are multiples of 64)
    D, _ = _wire_slabs(d, hid, pb=pb)
    assert all((getattr(D, f) - pb) % 128 == 0 for f in cols)


@pytest.mark.parametrize('d,hid', [(8, 32), (8, 24), (64, 384)])
def test_zero_buckets_store_and_accumulate_mode(d, hid):
    shared_n, exp_n = 6 * d + 4 * d * d + 4 * d, 2 * hid * d + hid + d

    def buckets():
        return [(torch.ones(shared_n), True, False), (torch.ones(exp_n), True, True), (torch.ones(exp_n), True, True)]
    # store mode: only the vector regions (the column folds accumulate into them); the matrices are written by the launches
    acq = buckets()
    engine._zero_buckets(acq, True, d, hid)
    want_s, want_e = torch.ones(shared_n), torch.ones(exp_n)
    want_s[:6 * d] = 0
    want_s[6 * d + 4 * d * d:] = 0
    want_e[hid * d:hid * d + hid] = 0
    want_e[2 * hid * d + hid:] = 0
    assert torch.equal(acq[0][0], want_s) and torch.equal(acq[1][0], want_e) and torch.equal(acq[2][0], want_e)
    # accumulate mode: a fresh bucket is zeroed whole, one that an earlier pass fed is left alone
    acq = buckets()
    acq[1] = (acq[1][0], False, True)
    engine._zero_buckets(acq, False, d, hid)
    assert not acq[0][0].any() and bool((acq[1][0] == 1).all()) and not acq[2][0].any()


def _km(plan):
    return None if plan.keymask is None else plan.keymask.tolist()


def test_plan_keymask_with_one_mask_or_one_modality():
    B, T, P = 2, 3, 2
    txt = torch.tensor([[1, 0, 1], [0, 1, 1]])
    img = torch.tensor([[1, 0], [1, 1]])
    lens = (2, 3)
    # one mask given: the other modality's rows are all valid
    p = engine.Plan(B, T, P, 'cpu', txt, None)
    assert _km(p) == [1, 0, 1, 0, 1, 1] + [1, 1, 1, 1] and (p.nt, p.ni, p.M, p.maxT) == (6, 4, 10, 3)
    assert _km(engine.Plan(B, T, P, 'cpu', None, img)) == [1] * 6 + [1, 0, 1, 1]
    assert _km(engine.Plan(B, T, P, 'cpu', txt, img)) == [1, 0, 1, 0, 1, 1] + [1, 0, 1, 1]
    assert _km(engine.Plan(B, T, P, 'cpu', None, None)) is None
    # ... the same with text lengths: sample 0 keeps positions 0, 1 and sample 1 all three
    p = engine.Plan(B, T, P, 'cpu', txt, None, txt_lens=lens)
    assert _km(p) == [1, 0, 0, 1, 1] + [1, 1, 1, 1] and (p.nt, p.ni, p.M, p.maxT) == (5, 4, 9, 3)
    assert _km(engine.Plan(B, T, P, 'cpu', None, img, txt_lens=lens)) == [1] * 5 + [1, 0, 1, 1]
    assert _km(engine.Plan(B, T, P, 'cpu', txt, img, txt_lens=lens)) == [1, 0, 0, 1, 1] + [1, 0, 1, 1]
    assert _km(engine.Plan(B, T, P, 'cpu', None, None, txt_lens=lens)) is None
    # a pass without text / without images
    p = engine.Plan(B, 0, P, 'cpu', None, img)
    assert _km(p) == [1, 0, 1, 1] and (p.nt, p.ni, p.M, p.maxT) == (0, 4, 4, 0) and p.seg_txt is None
    p = engine.Plan(B, T, 0, 'cpu', txt, None)
    assert _km(p) == [1, 0, 1, 0, 1, 1] and (p.nt, p.ni, p.M, p.maxT) == (6, 0, 6, 3) and p.seg_img is None
    p = engine.Plan(B, T, 0, 'cpu', txt, None, txt_lens=lens)
    assert _km(p) == [1, 0, 0, 1, 1] and (p.nt, p.ni, p.M, p.maxT) == (5, 0, 5, 3) and p.seg_img is None
    for p in (engine.Plan(B, 0, P, 'cpu', None, img), engine.Plan(B, T, 0, 'cpu', txt, None, txt_lens=lens)):
        assert p.keymask.dtype == torch.int32 and p.keymask.is_contiguous() and p.keymask.numel() == p.M
