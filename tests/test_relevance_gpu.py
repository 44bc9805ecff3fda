"""vlmo_relevance_step (csrc/relevance.hip) against fp64 on the CPU:
x_out[s, r, c0 + j] = alpha x_in[s, r, c0 + j] + beta sum_{k < n} x_in[s, r, c0 + k] A[s, k, j].

Exact cases: A in {0, 1} at density 0.05 with alpha = beta = 1, and A in {0, 2^-3} with alpha = beta = 0.5, x small
integers, two chained steps.  Every product, partial sum and result is then an integer multiple of one power of two (2^0,
resp. 2^-8 after the second step) and stays below 2^24 of them -- asserted on the fp64 result -- so fp32 arithmetic is
exact in any order and the kernel must give the fp64 chain bit for bit.

Bounded cases: non-negative inputs, so no cancellation.  One step is n products, n - 1 additions, two scalings and an
addition: at most n + 2 roundings of 2^-24 each on a chain whose terms are all >= 0; the bound doubles that, because the
inner accumulation of an MFMA is not documented to round to nearest at every step: per element, a chain of L steps is held
to a RELATIVE error of L (n + 3) 2^-23 against the fp64 chain on the same fp32 inputs, and to exactly 0 wherever fp64 is 0.
Nonzero entries of A are in [2^-6, 1] / n at 30 % density (one all-zero column, one all-zero row), x likewise in
[2^-6, 1]: no product underflows, and a dropped or doubled term moves a result by about 1 / (0.3 n) of itself or more,
three orders above the bound."""
import functools

import pytest
import torch

from exploremultimodal_amd import attnmap, hip

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = -7.5


def _ref_step(A, x, c0, alpha, beta):
    """fp64 statement of one step on CPU tensors (A [S, n, n], x [S, nq, width])."""
    n = A.shape[1]
    y = x.clone()
    y[:, :, c0:c0 + n] = alpha * x[:, :, c0:c0 + n] + beta * torch.einsum('srk,skj->srj', x[:, :, c0:c0 + n], A)
    return y


@functools.lru_cache(maxsize=None)
def _exact_inputs(S, nq, width, n, unit):
    """(A1, A2 fp32 [S, n, n] with entries in {0, unit} at density 0.05, x fp32 [S, nq, width] of integers in [0, 3]);
    on the CPU, shared, never modified.  A few entries of a small A are forced so that it is not all zero."""
    g = torch.Generator().manual_seed(7 * n + 31 * nq + S)
    As = []
    for _ in range(2):
        A = (torch.rand(S, n, n, generator=g) < 0.05).float() * unit
        A[:, n // 2, (n - 1) // 3] = unit
        A[:, 0, n - 1] = unit
        As.append(A)
    x = torch.randint(0, 4, (S, nq, width), generator=g).float()
    x[:, nq - 1, width - 1] = 3.0
    return As[0], As[1], x


def _exact_case(S, nq, width, c0, n):
    for unit, alpha, beta, lsb in ((1.0, 1.0, 1.0, 1.0), (2.0 ** -3, 0.5, 0.5, 2.0 ** -8)):
        A1, A2, x = _exact_inputs(S, nq, width, n, unit)
        want = _ref_step(A2.double(), _ref_step(A1.double(), x.double(), c0, alpha, beta), c0, alpha, beta)
        assert want.max().item() / lsb < 2 ** 24 and torch.equal(want / lsb, (want / lsb).round())
        assert (want[:, :, c0:c0 + n] != alpha * alpha * x[:, :, c0:c0 + n].double()).any(), 'the products are all zero'
        y1 = attnmap.relevance_step(A1.to(DEV), x.to(DEV), c0, alpha, beta)
        y2 = attnmap.relevance_step(A2.to(DEV), y1, c0, alpha, beta)
        assert y2.dtype == torch.float32 and y2.shape == x.shape
        bad = (y2.cpu().double() != want).sum().item()
        assert bad == 0, (f'{bad} of {want.numel()} elements differ from fp64 (S={S} nq={nq} width={width} c0={c0} n={n} '
                          f'alpha={alpha}); max |diff| {(y2.cpu().double() - want).abs().max().item():.3g}')


@pytest.mark.parametrize('n', [1, 17, 32, 33, 64, 65, 261])
def test_exact_full_width(n):
    for nq in sorted({1, 5, 33, n}):
        for S in (1, 5):
            _exact_case(S, nq, n, 0, n)


@pytest.mark.parametrize('c0,n,width', [(0, 9, 26), (9, 17, 26)])
def test_exact_column_ranges(c0, n, width):
    for nq in sorted({1, 5, 33, n}):
        for S in (1, 5):
            _exact_case(S, nq, width, c0, n)


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize('S,nq,width,c0,n', [(5, 33, 26, 9, 17), (2, 5, 26, 0, 9), (3, 65, 65, 0, 65), (1, 1, 1, 0, 1),
                                             (2, 70, 300, 20, 261)])
def test_untouched_memory(S, nq, width, c0, n):
    """x_out prefilled with a sentinel inside a larger buffer with guard elements on both sides: after the call the
    columns outside [c0, c0 + n), and the guards, keep their bits; A and x_in are unchanged; the written range is right."""
    GUARD = 256
    g = torch.Generator().manual_seed(11)
    A = torch.rand(S, n, n, generator=g)
    x = torch.rand(S, nq, width, generator=g)
    Ad, xd = A.to(DEV), x.to(DEV)
    buf = torch.full((GUARD + S * nq * width + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[GUARD:GUARD + S * nq * width].view(S, nq, width)
    hip.relevance_step(Ad, xd, out, c0, 1.0, 1.0)
    torch.cuda.synchronize()
    sent = _bits(torch.tensor([SENTINEL]))[0].item()
    assert (_bits(buf[:GUARD]) == sent).all() and (_bits(buf[-GUARD:]) == sent).all(), 'a guard element was written'
    assert (_bits(out[:, :, :c0]) == sent).all() and (_bits(out[:, :, c0 + n:]) == sent).all(), 'outside the column range'
    assert torch.equal(Ad.cpu(), A) and torch.equal(xd.cpu(), x)
    want = _ref_step(A.double(), x.double(), c0, 1.0, 1.0)[:, :, c0:c0 + n]
    got = out[:, :, c0:c0 + n].cpu().double()
    assert ((got - want).abs() <= (n + 3) * 2.0 ** -23 * want).all()


@functools.lru_cache(maxsize=None)
def _bounded_inputs(S, n, nq):
    """Three maps A fp32 [S, n, n] and x fp32 [S, nq, n] as the module docstring describes them; CPU, shared."""
    g = torch.Generator().manual_seed(1000 + n)

    def draw(*shape):
        v = 2.0 ** -6 + (1 - 2.0 ** -6) * torch.rand(*shape, generator=g)
        return torch.where(torch.rand(*shape, generator=g) < 0.3, v, torch.zeros(()))
    As = []
    for i in range(3):
        A = draw(S, n, n) / n
        A[:, :, n // 3] = 0        # an all-zero column, the same in every map (a masked key)
        A[:, n // 2, :] = 0        # an all-zero row (a query whose keys are all masked)
        As.append(A)
    x = draw(S, nq, n)
    x[:, 0, n // 3] = 0            # stays exactly 0 through the chain: the column gets alpha x only
    return tuple(As), x


@pytest.mark.parametrize('n,L,nq', [(261, 12, 261), (965, 12, 64), (1024, 2, 1)])
@pytest.mark.parametrize('alpha,beta', [(1.0, 1.0), (0.5, 0.5)])
def test_bounded_chain(n, L, nq, alpha, beta):
    S = 2
    As, x = _bounded_inputs(S, n, nq)
    want = x.double()
    for i in range(L):
        want = _ref_step(As[i % 3].double(), want, 0, alpha, beta)
    Ad = [A.to(DEV) for A in As]
    got = x.to(DEV)
    for i in range(L):
        got = attnmap.relevance_step(Ad[i % 3], got, 0, alpha, beta)
    got = got.cpu().double()
    zero = want == 0
    assert zero.any()
    assert (got[zero] == 0).all(), 'nonzero where fp64 is exactly 0'
    rel = ((got - want).abs()[~zero] / want[~zero]).max().item()
    bound = L * (n + 3) * 2.0 ** -23
    print(f'n={n} L={L} nq={nq} alpha={alpha}: max relative error {rel:.3e} (bound {bound:.3e}), '
          f'{int(zero.sum())} exact zeros, values in [{want[~zero].min().item():.3e}, {want.max().item():.3e}]')
    assert rel <= bound


def test_two_runs_are_bitwise_equal():
    As, x = _bounded_inputs(2, 261, 261)
    A, xd = As[0].to(DEV), x.to(DEV)
    a = attnmap.relevance_step(A, xd, 0, 1.0, 1.0)
    b = attnmap.relevance_step(A, xd, 0, 1.0, 1.0)
    assert torch.equal(_bits(a), _bits(b))
    # the same rows as part of a shorter window: the chain over k does not depend on the grid
    c = attnmap.relevance_step(A, xd[:, 64:97].contiguous(), 0, 1.0, 1.0)
    assert torch.equal(_bits(c), _bits(a[:, 64:97].contiguous()))


def test_refusals_write_nothing():
    L = hip.lib()
    S, nq, width, n = 2, 3, 8, 5
    A = torch.rand(S, n, n, device=DEV)
    buf = torch.rand(4 * S * nq * width, device=DEV)
    x = buf[:S * nq * width]
    out = torch.full((S * nq * width,), SENTINEL, device=DEV)
    keep_x = buf.clone()
    stream = torch.cuda.current_stream().cuda_stream
    pA, px, po = A.data_ptr(), x.data_ptr(), out.data_ptr()
    nan, inf = float('nan'), float('inf')
    # (A, x_in, x_out, num_seq, nq, width, c0, n, alpha, beta)
    cases = {
        'null A': (None, px, po, S, nq, width, 0, n, 1.0, 1.0),
        'null x_in': (pA, None, po, S, nq, width, 0, n, 1.0, 1.0),
        'null x_out': (pA, px, None, S, nq, width, 0, n, 1.0, 1.0),
        'in place': (pA, px, px, S, nq, width, 0, n, 1.0, 1.0),
        'overlap': (pA, px, px + 4 * width, S, nq, width, 0, n, 1.0, 1.0),
        'num_seq 0': (pA, px, po, 0, nq, width, 0, n, 1.0, 1.0),
        'nq 0': (pA, px, po, S, 0, width, 0, n, 1.0, 1.0),
        'n 0': (pA, px, po, S, nq, width, 0, 0, 1.0, 1.0),
        'n 1025': (pA, px, po, S, nq, 1025, 0, 1025, 1.0, 1.0),
        'width 1025': (pA, px, po, S, nq, 1025, 0, n, 1.0, 1.0),
        'c0 -1': (pA, px, po, S, nq, width, -1, n, 1.0, 1.0),
        'c0 + n > width': (pA, px, po, S, nq, width, 4, n, 1.0, 1.0),
        'alpha nan': (pA, px, po, S, nq, width, 0, n, nan, 1.0),
        'beta inf': (pA, px, po, S, nq, width, 0, n, 1.0, inf),
        'alpha -inf': (pA, px, po, S, nq, width, 0, n, -inf, 1.0),
    }
    for name, a in cases.items():
        rc = L.vlmo_relevance_step(*a, stream)
        torch.cuda.synchronize()
        assert rc < 0, (name, rc)
        assert b'vlmo_relevance_step' in L.vlmo_last_error(), name
        assert (out == SENTINEL).all(), f'{name}: x_out was written'
        assert torch.equal(buf, keep_x), f'{name}: x_in (or the memory behind it) was written'
    # the python entry points refuse what they can see themselves
    with pytest.raises(ValueError):
        attnmap.relevance_step(A, x.view(S, nq, width), c0=4)
    with pytest.raises(ValueError):
        attnmap.relevance_step(A.double(), x.view(S, nq, width))
    with pytest.raises(RuntimeError, match='overlap'):
        hip.relevance_step(A, x.view(S, nq, width), x.view(S, nq, width), 0, 1.0, 1.0)
    # and the accepted call right after still works
    assert L.vlmo_relevance_step(pA, px, po, S, nq, width, 0, n, 1.0, 1.0, stream) == 0
    torch.cuda.synchronize()
    assert (out.view(S, nq, width)[:, :, :n] != SENTINEL).all() and (out.view(S, nq, width)[:, :, n:] == SENTINEL).all()
