"""Host replica of the element dropout hash (csrc/common.h hash32 / drop_half / drop_bits4 / drop_keep).

Every site that uses it -- the proj / fc2 residual epilogues, the fc1 GELU epilogue and its saved-derivative form,
VLMO_EPI_DGELU, vlmo_resid_bwd, vlmo_ln_resid_bwd (one and two segments) and the three embedding kernels -- indexes
groups of four consecutive elements of a row-major [M, N] matrix: group g = e >> 2 of element e = m * N + n, elements
2h and 2h + 1 of the group take the low / high 16 bits of drop_half(seed, g, h) = hash32(((2g + h) ^ lo(seed)) *
0x9E3779B9 + hi(seed)).  2g + h is e >> 1, so per element:

    keep(e) <=> (hash32((uint32(e >> 1) ^ lo(seed)) * 0x9E3779B9 + hi(seed)) >> 16 * (e & 1)) & 0xFFFF >= thresh

numpy uint64 arithmetic masked to 32 bits, like tests/attn_counter.py."""
import numpy as np
import torch

_M = np.uint64(0xFFFFFFFF)


def hash32(x):
    """csrc/common.h hash32 on uint64 arrays holding 32-bit values"""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _M
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _M
    return x ^ (x >> np.uint64(16))


def thresh_of(p):
    """(thresh, inv_keep) as exploremultimodal_amd.hip.drop_params(p, True) computes them (no package import here:
    the CPU test of this file must not need the built library)"""
    t = int(round(p * 65536))
    return t, 65536.0 / (65536 - t)


def keep_mask(seed, M, N, thresh, row0=0):
    """bool [M, N]: the keep mask of rows row0 .. row0 + M of a row-major matrix with N columns under `seed`"""
    seed &= 0xFFFFFFFFFFFFFFFF
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    e = (np.arange(M, dtype=np.uint64)[:, None] + np.uint64(row0)) * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :]
    i = (e >> np.uint64(1)) & _M
    bits = hash32(((((i ^ lo) & _M) * np.uint64(0x9E3779B9)) + hi) & _M)
    field = (bits >> (np.uint64(16) * (e & np.uint64(1)))) & np.uint64(0xFFFF)
    return torch.from_numpy(field >= np.uint64(thresh))
