"""Launch tables of the multi-tensor kernels (exploremultimodal_amd.mt), built on the CPU from made-up addresses and read
back: the chunking, the position of every VlmoTensorList field inside the uploaded block, the Adam arguments and the
bounded cache.  A wrong field here is a kernel writing through a wrong address, so it is pinned where no kernel runs."""
import ctypes

import pytest
import torch

from exploremultimodal_amd import mt, optim
from exploremultimodal_amd.mt import CHUNK

CPU = torch.device('cpu')
NUMEL = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]


def _addr(col, nt):
    """Made-up, distinct addresses of column `col`: never dereferenced."""
    return [(col + 1) * (1 << 40) + 4096 * t for t in range(nt)]


def _five(numel):
    nt = len(numel)
    cols = [_addr(k, nt) for k in range(4)]
    return cols, mt.Table(CPU, cols[0], cols[1], numel, m=cols[2], v=cols[3])


def test_chunk_is_what_optim_exports():
    assert optim.CHUNK is mt.CHUNK and CHUNK == 1 << 16


def test_chunking():
    chunk_tensor, chunk_start = mt.chunks(NUMEL)
    assert len(chunk_tensor) == len(chunk_start) == 0 + 1 + 1 + 1 + 2 + 3
    assert chunk_tensor == sorted(chunk_tensor)
    assert 0 not in chunk_tensor                                    # the zero-element tensor owns no chunk
    for t, n in enumerate(NUMEL):
        assert [s for c, s in zip(chunk_tensor, chunk_start) if c == t] == list(range(0, n, CHUNK))
    for c, s in zip(chunk_tensor, chunk_start):
        assert s < NUMEL[c]
    # the same through a table: what the kernels read
    _, tab = _five(NUMEL)
    nt = len(NUMEL)
    assert tab.n_chunks == tab.tl.n_chunks == len(chunk_tensor)
    assert tab.dev_c.dtype == torch.int32 and tab.dev_c.tolist() == chunk_tensor
    assert tab.dev_i[5 * nt:].tolist() == chunk_start


def test_five_column_table():
    (p, g, m, v), tab = _five(NUMEL)
    nt, tl = len(NUMEL), tab.tl
    assert tab.nt == nt
    base = tab.dev_i.data_ptr()
    for k, name in enumerate(('p', 'g', 'm', 'v', 'numel', 'chunk_start')):
        assert getattr(tl, name) == base + 8 * nt * k, name
    assert tab.dev_i.dtype == torch.int64 and tab.dev_i.numel() == 5 * nt + tab.n_chunks
    assert tab.dev_i[:5 * nt].tolist() == p + g + m + v + NUMEL
    assert tl.chunk_tensor == tab.dev_c.data_ptr()
    assert tl.lr == tab.dev_f.data_ptr() and tl.wd - tl.lr == 4 * nt
    assert tab.dev_f.dtype == torch.float32 and tab.dev_f.numel() == 2 * nt
    assert tab.partial.dtype == torch.float32 and tab.partial.numel() == tab.n_chunks
    assert tab.ctl.dtype == torch.float32 and tab.ctl.tolist() == [0.0] * 4
    assert tl.chunk == CHUNK
    # the g column is a view into the block: what a caller writes there is what tl.g points at
    assert tab.g.data_ptr() == tl.g and tab.g.tolist() == g
    tab.g.copy_(torch.tensor(_addr(7, nt)))
    assert tab.dev_i[nt:2 * nt].tolist() == _addr(7, nt)
    assert tab.dev_i[:nt].tolist() == p and tab.dev_i[2 * nt:3 * nt].tolist() == m


def test_three_column_table():
    nt = len(NUMEL)
    p, g = _addr(0, nt), _addr(1, nt)
    tab = mt.Table(CPU, p, g, NUMEL)
    tl = tab.tl
    for name in ('m', 'v', 'lr', 'wd'):
        assert getattr(tl, name) is None, name                    # NULL, not dummy storage
    assert tab.dev_f is None and tab.partial is None and tab.ctl is None
    base = tab.dev_i.data_ptr()
    for k, name in enumerate(('p', 'g', 'numel', 'chunk_start')):
        assert getattr(tl, name) == base + 8 * nt * k, name
    assert tab.dev_i[:3 * nt].tolist() == p + g + NUMEL
    assert tab.dev_i[3 * nt:].tolist() == mt.chunks(NUMEL)[1]
    assert tl.chunk_tensor == tab.dev_c.data_ptr()
    assert (tl.n_chunks, tl.chunk) == (0 + 1 + 1 + 1 + 2 + 3, CHUNK)


def test_empty_list():
    for tab in (mt.Table(CPU, [], [], []), mt.Table(CPU, [], [], [], m=[], v=[])):
        assert tab.nt == 0 and tab.n_chunks == 0 and tab.tl.n_chunks == 0
        assert tab.dev_i.numel() == 0 and tab.dev_c.numel() == 0 and tab.g.numel() == 0
    # the buffers a kernel is handed are never zero-sized
    assert tab.dev_f.numel() == 1 and tab.partial.numel() == 1 and tab.ctl.numel() == 4


def test_a_short_column_is_refused():
    with pytest.raises(ValueError, match='one entry per tensor'):
        mt.Table(CPU, [1 << 40], [], [5])


def _f32(x):
    return ctypes.c_float(x).value


@pytest.mark.parametrize('step', [1, 1000])
@pytest.mark.parametrize('bias_correction', [True, False])
def test_adam_args(step, bias_correction):
    b1, b2, eps = 0.9, 0.98, 1e-6
    for adam_w_mode in (True, False, 1, 0):
        a = mt.adam_args((b1, b2), eps, bias_correction, step, adam_w_mode)
        assert (a.beta1, a.beta2, a.eps) == (_f32(b1), _f32(b2), _f32(eps))
        if bias_correction:     # in double from the betas as given, rounded to fp32 once
            assert a.inv_bc1 == _f32(1.0 / (1.0 - b1 ** step)) and a.inv_bc2 == _f32(1.0 / (1.0 - b2 ** step))
        else:
            assert a.inv_bc1 == 1.0 and a.inv_bc2 == 1.0
        assert a.adam_w_mode == (1 if adam_w_mode else 0)


def test_bounded_cache():
    cache, made = {}, []

    def make_for(sig):
        def make():
            made.append(sig)
            return object()
        return make
    first = [mt.recent(cache, s, make_for(s)) for s in range(8)]
    assert made == list(range(8)) and list(cache) == list(range(8))
    for s in range(8):                                              # hits: the same object, make() not called
        assert mt.recent(cache, s, make_for(s)) is first[s]
    assert made == list(range(8))
    mt.recent(cache, 8, make_for(8))                                # the ninth evicts the first, and only the first
    assert list(cache) == list(range(1, 9))
    assert all(cache[s] is first[s] for s in range(1, 8))
    assert mt.recent(cache, 0, make_for(0)) is not first[0]
    assert made == list(range(9)) + [0] and list(cache) == list(range(2, 9)) + [0]
