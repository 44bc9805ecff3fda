"""Host-side check of the row ring of ln_bwd_kernel (csrc/layernorm.hip, LnRing), in the style of
tests/test_lds_layouts.py: the slot layout, the LDS-DMA placement (one wave-instruction writes 1 KB, lane l its bytes
[16 l, 16 l + 16); the lanes past a piece's end repeat the piece's last 16 bytes) and the lane's read-back addresses
are restated here as pure functions, and for every instantiation and width the byte a lane reads back is the byte of
the row it is meant to hold.  No GPU needed."""
import numpy as np
import pytest

WAVES = 4
LDS_PER_CU = 160 * 1024


def vpl_of(d):
    return (d // 4 + 63) // 64


def ring(vpl, dy_f32, resid):
    """LnRing: byte offsets of the pieces of a slot, the slot, the slots per wave, the workgroup's bytes"""
    half, full = ((vpl + 1) // 2) * 1024, vpl * 1024
    off = {'dy': 0}
    off['x'] = full if dy_f32 else half
    off['dr'] = off['x'] + full
    off['z'] = off['dr'] + full
    slot = off['z'] + (half if resid else 0)
    nslot = 2 if 8 * slot <= 80 * 1024 else 1
    return off, slot, nslot, WAVES * nslot * slot


def pieces(vpl, d, dy_f32, resid):
    """name -> (bytes of the row piece, element size, LDS-DMA instructions)"""
    p = {'dy': (4 * d, 4, vpl) if dy_f32 else (2 * d, 2, (vpl + 1) // 2), 'x': (4 * d, 4, vpl), 'dr': (4 * d, 4, vpl)}
    if resid:
        p['z'] = (2 * d, 2, (vpl + 1) // 2)
    return p


def dma_src(jj, lane, nb):
    """ring_piece: the byte offset in the row piece that instruction jj's lane fetches (16 bytes)"""
    return min(jj * 1024 + lane * 16, nb - 16)


def read_addr(j, lane, esize):
    """the lane's j-th vector of four elements: ds_read_b128 (fp32) / ds_read_b64 (bf16), offset inside the piece"""
    return j * 1024 + lane * 16 if esize == 4 else j * 512 + lane * 8


WIDTHS = [8, 192, 256, 264, 512, 520, 768, 776, 1024]
FORMS = [(False, True), (False, False), (True, False)]      # (DY_F32, RESID) of the three launches


@pytest.mark.parametrize('d', WIDTHS)
@pytest.mark.parametrize('dy_f32,resid', FORMS)
def test_ring_slot_holds_the_row(d, dy_f32, resid):
    vpl = vpl_of(d)
    off, slot, nslot, total = ring(vpl, dy_f32, resid)
    ps = pieces(vpl, d, dy_f32, resid)
    for wave in range(WAVES):
        for s in range(nslot):
            base = (wave * nslot + s) * slot
            assert base + slot <= total
            lds = np.full(total, -1, dtype=np.int64)            # per byte: piece id * 2^16 + byte offset in the piece
            owner = np.full(total, -1, dtype=np.int64)
            for pid, (name, (nb, esize, ni)) in enumerate(ps.items()):
                assert nb % 16 == 0 and nb >= 16
                assert ni * 1024 >= nb, 'the instructions cover the piece'
                for jj in range(ni):
                    for lane in range(64):
                        src = dma_src(jj, lane, nb)
                        assert 0 <= src and src + 16 <= nb, 'a lane reads outside its row'
                        dst = base + off[name] + jj * 1024 + lane * 16
                        assert base <= dst and dst + 16 <= base + slot, 'a lane writes outside its slot'
                        assert (owner[dst:dst + 16] == -1).all() or (owner[dst:dst + 16] == pid).all(), 'pieces overlap'
                        owner[dst:dst + 16] = pid
                        lds[dst:dst + 16] = pid * 65536 + src + np.arange(16)
            nv = d // 4
            for pid, (name, (nb, esize, ni)) in enumerate(ps.items()):
                for j in range(vpl):
                    for lane in range(64):
                        i = lane + 64 * j
                        a = base + off[name] + read_addr(j, lane, esize)
                        n = 4 * esize
                        assert a % n == 0 and a + n <= base + slot, 'a read leaves the slot'
                        if i < nv:
                            want = pid * 65536 + i * n + np.arange(n)
                            np.testing.assert_array_equal(lds[a:a + n], want)


@pytest.mark.parametrize('dy_f32,resid', FORMS)
def test_ring_budget(dy_f32, resid):
    """two workgroups per CU: ring <= 80 KB; two slots up to VPL = 3, and at VPL = 4 whenever they fit"""
    for vpl in (1, 2, 3, 4):
        off, slot, nslot, total = ring(vpl, dy_f32, resid)
        red = WAVES * (4 if resid else 2) * vpl * 256 * 4         # the column fold that aliases the ring afterwards
        assert 2 * max(total, red) <= LDS_PER_CU
        assert slot <= 10 * 1024 or nslot == 1
        if vpl <= 3:
            assert nslot == 2
    assert ring(3, False, True)[1:] == (10 * 1024, 2, 80 * 1024)
    assert ring(4, False, True)[1:] == (12 * 1024, 1, 48 * 1024)


def test_wait_counts():
    """The counted wait of row k leaves in flight exactly what was issued after row k's fetch.  Replay of the loop's
    issue order for every row count: fetch(0..NSLOT-1); then per row k: wait, [fetch(k + NSLOT)], stores(k)."""
    for nslot in (1, 2):
        for nfetch, stores in ((10, 6), (7, 3), (4, 2)):
            for nrow in range(0, 12):
                queue = []                                        # issue order, oldest first
                for s in range(min(nslot, nrow)):
                    queue += [('f', s)] * nfetch
                for k in range(nrow):
                    younger = min(k, nslot) * stores + sum(nfetch for t in range(1, nslot) if k + t < nrow)
                    last = max(i for i, op in enumerate(queue) if op == ('f', k))
                    assert len(queue) - 1 - last == younger, (nslot, nrow, k)
                    if k + nslot < nrow:
                        queue += [('f', k + nslot)] * nfetch
                    queue += [('s', k)] * stores
