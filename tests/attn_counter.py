"""Host replica of the attention-dropout counter (csrc/attention.hip att_key / att_stride / att_mix).

keep(seq, head, q, key) <=> top 16 bits of mix((q * S(N) + key) * G + key(seed, (mask_seq0 + seq) * heads + head)) >= thresh,
where N is the SEQUENCE's own length: S(N) = 512 for N <= 512 (the counter of the resident kernels, bit for bit) and
1024 above (collision-free up to 1024 tokens)."""
import numpy as np
import torch

from tests.dropmask import hash32 as _hash32

_M = np.uint64(0xFFFFFFFF)


def stride(n):
    return 512 if n <= 512 else 1024


def counter(q, key, n):
    """the 32-bit counter of (q, key) in a sequence of n tokens (numpy arrays or ints)"""
    return (np.asarray(q, dtype=np.uint64) * np.uint64(stride(n)) + np.asarray(key, dtype=np.uint64)) & _M


def keep_mask(seed, lens, heads, thresh, npad=None, seq0=0):
    """[len(lens), heads, npad, npad] bool keep mask of the sequences of one launch (rows / columns past a sequence's
    own length are True and unused)"""
    npad = npad or max(lens)
    out = torch.ones(len(lens), heads, npad, npad, dtype=torch.bool)
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for s, n in enumerate(lens):
        c = counter(np.arange(n)[:, None], np.arange(n)[None, :], n)
        for hd in range(heads):
            bh = np.uint64((seq0 + s) * heads + hd)
            akey = (_hash32((lo ^ ((bh * np.uint64(0x9E3779B9)) & _M)) & _M) + hi) & _M
            x = ((c * np.uint64(0x9E3779B1)) + akey) & _M
            x = x ^ (x >> np.uint64(15))
            x = (x * np.uint64(0x7feb352d)) & _M
            out[s, hd, :n, :n] = torch.from_numpy((x >> np.uint64(16)) >= np.uint64(thresh))
    return out
