"""The attention-dropout counter rule for sequences of up to 1024 tokens (tests/attn_counter.py replicates
csrc/attention.hip): unchanged for sequences of <= 512 tokens, collision-free above."""
import numpy as np
import pytest

from tests import attn_counter


@pytest.mark.parametrize('n', [1, 40, 64, 197, 261, 288, 289, 500, 512])
def test_counter_is_the_resident_kernels_counter_up_to_512_tokens(n):
    q, k = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    assert np.array_equal(attn_counter.counter(q, k, n), (q * 512 + k).astype(np.uint64))


@pytest.mark.parametrize('n', [513, 577, 593, 641, 700, 901, 941, 965, 1024])
def test_counter_is_collision_free_above_512_tokens(n):
    q, k = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    c = attn_counter.counter(q, k, n).ravel()
    assert np.unique(c).size == n * n
    # the 512-stride counter aliased here: (q, key + 512) and (q + 1, key) shared one keep decision
    assert np.unique((q * 512 + k).ravel()).size < n * n


def test_stride_follows_the_sequence_not_the_launch():
    """a 40-token text sequence keeps the 512 stride whatever launch it rides in (a 577-token forward launch, a
    40-token backward launch): the mask depends on (seed, sequence index, its own length) only"""
    a = attn_counter.keep_mask(7, [577, 40], 1, 6554)
    b = attn_counter.keep_mask(7, [40], 1, 6554, seq0=1)
    assert np.array_equal(a[1, :, :40, :40].numpy(), b[0].numpy())
    assert attn_counter.stride(40) == 512 and attn_counter.stride(577) == 1024
