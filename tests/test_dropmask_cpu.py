"""Statistics and indexing of the host replica of the element dropout hash (tests/dropmask.py): what a mask that the
GPU tests hand to their references must satisfy whatever the kernels do."""
import math

import pytest
import torch

from tests import dropmask

SEEDS = [1234, 0x1234567ABCDEF01, 99, 2 ** 62 - 5]
SHAPES = [(300, 128), (77, 384), (1024, 1024)]
THRESH = round(0.1 * 65536)


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('M,N', SHAPES)
def test_drop_rate_is_within_four_sigma_of_p(seed, M, N):
    keep = dropmask.keep_mask(seed, M, N, THRESH)
    assert keep.shape == (M, N) and keep.dtype == torch.bool
    rate = 1.0 - keep.float().mean().item()
    sigma = math.sqrt(0.09 / (M * N))
    print(f'seed {seed:#x} ({M}, {N}): drop rate {rate:.5f}, bound 0.1 +- {4 * sigma:.5f}')
    assert abs(rate - 0.1) <= 4 * sigma, (rate, 4 * sigma)


@pytest.mark.parametrize('seed', SEEDS)
def test_seeds_one_apart_give_unrelated_masks(seed):
    """two independent masks of rate p differ in 2 p (1 - p) = 18 % of the elements"""
    M, N = 300, 128
    a, b = dropmask.keep_mask(seed, M, N, THRESH), dropmask.keep_mask(seed + 1, M, N, THRESH)
    diff = (a != b).float().mean().item()
    print(f'seeds {seed:#x} / +1 differ in {100 * diff:.2f} % of the elements')
    assert 0.16 <= diff <= 0.20, diff


@pytest.mark.parametrize('M,N,r', [(300, 128, 1), (77, 384, 13), (77, 132, 50), (1024, 1024, 1000)])
def test_row0_is_a_row_offset_into_the_same_stream(M, N, r):
    seed = SEEDS[1]
    full = dropmask.keep_mask(seed, M, N, THRESH)
    assert torch.equal(dropmask.keep_mask(seed, M - r, N, THRESH, row0=r), full[r:])


def test_thresh_zero_keeps_everything_and_thresh_of_matches_the_rate():
    assert dropmask.keep_mask(5, 16, 8, 0).all()
    t, inv = dropmask.thresh_of(0.1)
    assert t == THRESH and abs(inv - 65536.0 / (65536 - THRESH)) < 1e-12


def test_scalar_walk_of_the_device_code_agrees():
    """the same rule written the way csrc/common.h writes it (group index, half, 64-bit field), element by element"""
    def h32(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        return x ^ (x >> 16)

    seed, M, N, row0 = 0x1234567ABCDEF01, 5, 12, 3
    got = dropmask.keep_mask(seed, M, N, THRESH, row0=row0)
    for m in range(M):
        for n in range(0, N, 4):
            g = ((row0 + m) * N + n) >> 2
            half = [h32((((2 * g + h) & 0xFFFFFFFF ^ (seed & 0xFFFFFFFF)) * 0x9E3779B9 + (seed >> 32)) & 0xFFFFFFFF) for h in (0, 1)]
            bits = half[0] | (half[1] << 32)
            for j in range(4):
                assert bool(got[m, n + j]) == (((bits >> (16 * j)) & 0xFFFF) >= THRESH), (m, n, j)
