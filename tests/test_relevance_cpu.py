"""Relevance over the depth (attnmap.relevance_*) without a GPU: the torch statement of the definition against Chefer, Gur
and Wolf's rule computed by autograd on a hand-written attention stack, the algebra of ``queries`` and ``layers``, the
rollout row sums, the zero rules of masked keys, the argument errors, the heat-map shapes and the ctypes binding.

The stack: 3 layers, 2 heads, head width 4; per layer P = softmax(q k^T / 2 + keymask) is re-made a leaf with
requires_grad (so that P.grad is d score / d P with P a free variable of ctx = P v), x <- x + concat_h(P_h v_h) W_o.  Chefer's
rule is then stated directly: Abar = clamp(P.grad * P, 0).mean(heads), R <- R + Abar R from layer 0 upward, R = I at the
start.  Both sides are fp64 and run the same products in the same order up to the blockdiag assembly, so they agree to
1e-12 (values are O(1))."""
import math
import os
import re

import pytest
import torch

from exploremultimodal_amd import attnmap, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS, HD, DEPTH = 2, 4, 3
D = HEADS * HD


def _weights(seed):
    g = torch.Generator().manual_seed(seed)
    return [{n: torch.randn(D, D, generator=g, dtype=torch.float64) * 0.5 for n in ('q', 'k', 'v', 'o')}
            for _ in range(DEPTH)]


def _attend(x, w, keep):
    """x [B, n, D], keep [B, n] bool -> (x + attention output, P leaf [B, HEADS, n, n])."""
    B, n, _ = x.shape
    q, k, v = ((x @ w[m]).view(B, n, HEADS, HD).transpose(1, 2) for m in ('q', 'k', 'v'))
    s = (q @ k.transpose(-1, -2)) / 2.0
    s = s.masked_fill(~keep[:, None, None, :], float('-inf'))
    P = s.softmax(-1).detach().requires_grad_(True)
    ctx = (P @ v).transpose(1, 2).reshape(B, n, D)
    return x + ctx @ w['o'], P


def _stack(x, keep, T, fusion):
    """The stack on x [B, N, D]: layers below ``fusion`` attend tokens [0, T) and [T, N) separately (T = None: one
    modality).  Returns {layer: head-mean cam map or {'txt', 'img'} dict, [B, 1, n, n]} and Chefer's R [B, N, N]."""
    ws = _weights(5)
    B, N, _ = x.shape
    leaves = []
    for i, w in enumerate(ws):
        if T is not None and i < fusion:
            xt, Pt = _attend(x[:, :T], w, keep[:, :T])
            xi, Pi = _attend(x[:, T:], w, keep[:, T:])
            x = torch.cat([xt, xi], dim=1)
            leaves.append({'txt': Pt, 'img': Pi})
        else:
            x, P = _attend(x, w, keep)
            leaves.append(P)
    score = (x[:, 0] * torch.linspace(-1, 1, D, dtype=torch.float64)).sum() + x[:, -1].sum()
    score.backward()

    def cam(P):
        return (P.grad * P.detach()).clamp_min(0).mean(1, keepdim=True)

    maps, R = {}, torch.eye(N, dtype=torch.float64).expand(B, N, N).clone()
    for i, leaf in enumerate(leaves):
        if isinstance(leaf, dict):
            maps[i] = {n: cam(P) for n, P in leaf.items()}
            Abar = torch.zeros(B, N, N, dtype=torch.float64)
            Abar[:, :T, :T], Abar[:, T:, T:] = maps[i]['txt'][:, 0], maps[i]['img'][:, 0]
        else:
            maps[i] = cam(leaf)
            Abar = maps[i][:, 0]
        R = R + Abar @ R
    return maps, R


def _case(N, T, fusion, masked=()):
    g = torch.Generator().manual_seed(100 + N)
    x = torch.randn(2, N, D, generator=g, dtype=torch.float64)
    keep = torch.ones(2, N, dtype=torch.bool)
    for b, j in masked:
        keep[b, j] = False
    return _stack(x, keep, T, fusion)


@pytest.mark.parametrize('N,T,fusion', [(7, None, 0), (7, 3, 1)])
def test_reference_is_chefers_rule_by_autograd(N, T, fusion):
    maps, R = _case(N, T, fusion)
    assert isinstance(maps[0], dict) == (T is not None)
    got = attnmap.relevance_reference(maps, N, T, method='gradcam', dtype=torch.float64)
    assert got.shape == (2, N, N) and got.dtype == torch.float64
    assert (R - torch.eye(N, dtype=torch.float64)).abs().max() > 1e-3           # the maps carry gradient
    err = (got - R).abs().max().item()
    print(f'max |relevance_reference - autograd Chefer| = {err:.3g}')
    assert err <= 1e-12
    # the row form through relevance_step (CPU restatement) is the same matrix
    X = attnmap.relevance_rows(2, N, 0, N, 'cpu', torch.float64)
    for i in reversed(sorted(maps)):
        X = attnmap.relevance_propagate(X, maps[i], T, 1.0, 1.0)
    assert (X - R).abs().max().item() <= 1e-12


def test_queries_are_row_slices_and_layers_a_sub_product():
    maps, _ = _case(7, 3, 1)
    full = attnmap.relevance_reference(maps, 7, 3, dtype=torch.float64)
    for q0, nq in ((0, 1), (2, 3), (6, 1), (0, 7)):
        win = attnmap.relevance_reference(maps, 7, 3, queries=(q0, nq), dtype=torch.float64)
        assert win.shape == (2, nq, 7) and torch.equal(win, full[:, q0:q0 + nq])
    eye = torch.eye(7, dtype=torch.float64)

    def factor(m, alpha, beta):
        A = torch.zeros(2, 7, 7, dtype=torch.float64)
        if isinstance(m, dict):
            A[:, :3, :3], A[:, 3:, 3:] = m['txt'][:, 0], m['img'][:, 0]
        else:
            A = m[:, 0]
        return alpha * eye + beta * A
    for method, (alpha, beta) in (('gradcam', (1.0, 1.0)), ('rollout', (0.5, 0.5))):
        for sub in ([0, 2], [1], [0, 1, 2]):
            want = eye.expand(2, 7, 7)
            for i in sub:                                    # top layer leftmost
                want = factor(maps[i], alpha, beta) @ want
            got = attnmap.relevance_reference({i: maps[i] for i in sub}, 7, 3, method=method, dtype=torch.float64)
            assert (got - want).abs().max().item() <= 1e-12, (method, sub)


def _softmax_maps(L, n, masked):
    """L row-stochastic maps [2, 1, n, n] with the key columns ``masked`` exactly 0."""
    g = torch.Generator().manual_seed(3)
    s = torch.randn(L, 2, 1, n, n, generator=g, dtype=torch.float64)
    s[..., list(masked)] = float('-inf')
    return {i: s[i].softmax(-1) for i in range(L)}


def test_rollout_rows_sum_to_one():
    L, n = 4, 9
    maps = _softmax_maps(L, n, masked=(4,))
    R = attnmap.relevance_reference(maps, n, method='rollout', dtype=torch.float64)
    dev = (R.sum(-1) - 1).abs().max().item()
    print(f'max |row sum - 1| = {dev:.3g} (bound {L * n * 2.0 ** -50:.3g})')
    assert dev <= L * n * 2.0 ** -50
    assert (R >= 0).all()


@pytest.mark.parametrize('method', ['gradcam', 'rollout'])
def test_masked_key_column_holds_the_identity_part_only(method):
    alpha = attnmap.METHODS[method][0]
    if method == 'rollout':
        L, n, col = 4, 9, 4
        maps = _softmax_maps(L, n, masked=(col,))
        R = attnmap.relevance_reference(maps, n, method=method, dtype=torch.float64)
    else:
        L, n, col = DEPTH, 7, 5
        maps, _ = _case(7, 3, 1, masked=((0, col), (1, col)))
        for m in maps.values():
            for A in (m.values() if isinstance(m, dict) else [m]):
                assert (A >= 0).all()
        R = attnmap.relevance_reference(maps, n, 3, method=method, dtype=torch.float64)
    want = torch.zeros(n, dtype=torch.float64)
    want[col] = alpha ** L
    assert torch.equal(R[:, :, col], want.expand(2, n))
    assert (R[:, :, :col] > 0).any() and (R >= 0).all()
    # a query row whose keys are all masked (a zero row of every map) propagates alpha X only
    zero_row = {i: m.clone() for i, m in _softmax_maps(3, 6, masked=()).items()}
    for m in zero_row.values():
        m[:, :, 2, :] = 0
    R = attnmap.relevance_reference(zero_row, 6, method=method, dtype=torch.float64)
    want = torch.zeros(6, dtype=torch.float64)
    want[2] = alpha ** 3
    assert torch.equal(R[:, 2], want.expand(2, 6))


def test_relevance_step_restatement_and_column_ranges():
    g = torch.Generator().manual_seed(9)
    A = torch.rand(3, 17, 17, generator=g, dtype=torch.float64)
    x = torch.rand(3, 5, 26, generator=g, dtype=torch.float64)
    y = attnmap.relevance_step(A, x, c0=9, alpha=0.5, beta=0.25)
    assert y is not x and y.shape == x.shape
    assert torch.equal(y[:, :, :9], x[:, :, :9])
    want = 0.5 * x[:, :, 9:] + 0.25 * torch.einsum('srk,skj->srj', x[:, :, 9:], A)
    assert (y[:, :, 9:] - want).abs().max().item() <= 1e-14
    assert torch.equal(attnmap.relevance_step(A, x[:, :, 9:].contiguous()), x[:, :, 9:] + x[:, :, 9:] @ A)


def test_argument_errors():
    maps, _ = _case(7, 3, 1)
    with pytest.raises(ValueError, match='method'):
        attnmap.relevance_reference(maps, 7, 3, method='chefer')
    for bad in ((-1, 2), (0, 0), (5, 3), (7, 1)):
        with pytest.raises(ValueError, match='queries'):
            attnmap.relevance_reference(maps, 7, 3, queries=bad)
    with pytest.raises(ValueError):
        attnmap.relevance_reference(maps, 8, 3)                                 # the maps have 7 tokens
    with pytest.raises(ValueError):
        attnmap.relevance_reference(maps, 7, 4)                                 # the text block has 3
    with pytest.raises(ValueError):
        attnmap.relevance_reference({}, 7)
    with pytest.raises(ValueError):
        attnmap.relevance_reference({0: torch.rand(2, 2, 7, 7)}, 7)             # per-head maps: head_mean=True is needed
    with pytest.raises(ValueError):
        attnmap.relevance_reference({0: torch.rand(2, 1, 3, 7)}, 7)             # a query window of the map
    A, x = torch.rand(2, 4, 4), torch.rand(2, 3, 6)
    for c0 in (-1, 3):
        with pytest.raises(ValueError, match='columns'):
            attnmap.relevance_step(A, x, c0=c0)
    with pytest.raises(ValueError):
        attnmap.relevance_step(A[:1], x)
    with pytest.raises(ValueError):
        attnmap.relevance_step(torch.rand(2, 4, 5), x)
    assert attnmap.check_layers(None, 3) == [0, 1, 2] and attnmap.check_layers((0, 2), 3) == [0, 2]
    for bad in ([1, 0], [0, 0], [3], [-1]):
        with pytest.raises(ValueError, match='layers'):
            attnmap.check_layers(bad, 3)


def test_heatmap_shapes():
    B, nq, T, grid = 2, 3, 5, 4
    R = torch.arange(B * nq * (T + 1 + grid * grid), dtype=torch.float32).view(B, nq, -1)
    txt, img = attnmap.relevance_heatmaps(R, T, grid)
    assert txt.shape == (B, nq, T) and img.shape == (B, nq, grid, grid)
    assert torch.equal(txt, R[:, :, :T]) and torch.equal(img.reshape(B, nq, -1), R[:, :, T + 1:])      # column T left out
    txt, img = attnmap.relevance_heatmaps(R[:, :, T:], 0, grid)                                     # an image-only pass
    assert txt.shape == (B, nq, 0) and torch.equal(img.reshape(B, nq, -1), R[:, :, T + 1:])
    with pytest.raises(ValueError):
        attnmap.relevance_heatmaps(R, T + 1, grid)


def test_binding_has_the_headers_argument_count():
    header = open(os.path.join(ROOT, 'include', 'vlmo_hip.h')).read()
    m = re.search(r'\bint\s+vlmo_relevance_step\s*\(([^)]*)\)\s*;', header)
    assert m, 'vlmo_relevance_step is not declared in include/vlmo_hip.h'
    nargs = len([a for a in m.group(1).split(',') if a.strip()])
    assert nargs == 11
    assert len(hip._SIGS['vlmo_relevance_step']) == nargs
    assert 'vlmo_relevance_step' in hip.exported_symbols() and callable(hip.relevance_step)
    assert math.isclose(attnmap.METHODS['rollout'][0], 0.5) and attnmap.METHODS['gradcam'] == (1.0, 1.0)
