"""The launch plan of vlmo_gemm_tn_multi (csrc/tn_multi_plan.h), read through the host query vlmo_gemm_tn_multi_plan:
no GPU.  `restate` below is the plan's rules written down a second time, from their description and without the
library; the query must equal it field for field and table for table on the training shapes and on the lists of the
GPU tests.  The placement properties are then asserted on the query's tables directly."""
import os
from collections import Counter

import pytest

from exploremultimodal_amd import hip

ATOMIC, ACCUM, STORE = 0, 1, 2
NOP = 0xFFFF


class PlanError(Exception):
    pass


def _cdiv(a, b):
    return -(-a // b)


def restate(shapes):
    """[(M, N1, N2, accumulate)] -> the launches, in the form hip.gemm_tn_multi_plan returns."""
    launches, q0 = [], 0
    while q0 < len(shapes):
        nq = T = 0                  # chunking: < 16 problems, <= 960 tiles of 256 x 256; the first is always taken
        while q0 + nq < len(shapes) and nq < 16:
            t = _cdiv(shapes[q0 + nq][1], 256) * _cdiv(shapes[q0 + nq][2], 256)
            if nq > 0 and T + t > 960:
                break
            T, nq = T + t, nq + 1
        chunk = shapes[q0:q0 + nq]
        nk_min = min(_cdiv(M, 64) for M, _, _, _ in chunk)
        splits = 1 if T >= 192 else max(1, min(256 // T, nk_min // 8))
        problems, jobs = [], []
        for q, (M, N1, N2, acc) in enumerate(chunk):
            tiles, nk = _cdiv(N1, 256) * _cdiv(N2, 256), _cdiv(M, 64)
            sp = min(splits, nk)
            per = _cdiv(nk, sp)
            sp = _cdiv(nk, per)
            if tiles * sp > 4096:
                raise PlanError('too many tiles')
            mode = ATOMIC if sp > 1 else ACCUM if acc else STORE
            problems.append((tiles, sp, per, mode, int(sp > 1 and not acc)))
            jobs += [((q << 12) | l, per) for l in range(tiles * sp)]
        jobs.sort(key=lambda j: -j[1])          # stable: equal costs keep (problem, workgroup) order
        bins = [[] for _ in range(8)]
        i = 0
        while i < len(jobs):                    # every run of equal cost is dealt to the 8 XCDs in contiguous pieces
            j = i
            while j < len(jobs) and jobs[j][1] == jobs[i][1]:
                j += 1
            for x in range(8):
                bins[x] += [code for code, _ in jobs[i + (j - i) * x // 8:i + (j - i) * (x + 1) // 8]]
            i = j
        grid = 8 * max(len(b) for b in bins)
        if grid > 1024:
            raise PlanError('exceed one launch')
        order = [bins[b & 7][b >> 3] if (b >> 3) < len(bins[b & 7]) else NOP for b in range(grid)]
        launches.append(dict(q0=q0, nq=nq, problems=problems, grid=grid, order=order))
        q0 += nq
    return launches


def _blocks(M_rows, d, hidden, nblk=2):
    """Weight-gradient problems of nblk blocks, each with one attention and one FFN per row count of M_rows[1:] (or of
    M_rows[0] when there is one), longest reductions first as the backward pass submits them."""
    per = [(M_rows[0], d, d), (M_rows[0], 3 * d, d)]
    for M in M_rows[1:] or M_rows[:1]:
        per += [(M, d, hidden), (M, hidden, d)]
    return sorted(per * nblk, key=lambda s: -s[0])


def _gpu_test_lists():
    small = [(700, 256, 512, 1), (333, 96, 264, 0), (1000, 512, 256, 1)]
    big = [(300, 768, 3072, 1), (200, 3072, 768, 0), (130, 768, 768, 1), (257, 2304, 768, 1), (64, 1000, 264, 0)]
    many = [(64 + 8 * i, 256, 264, 1) for i in range(19)]
    wide = [(64 * (1 + i % 3) + (5 if i % 4 == 0 else 0), 2048, 2048, int(i % 2 == 0)) for i in range(20)]
    return {'gpu_small': small, 'gpu_big': big, 'gpu_19_problems': many, 'gpu_20x64_tiles': wide}


LISTS = {
    **{f'base_two_experts_acc{a}': [s + (a,) for s in _blocks([16704, 4096, 12608], 768, 3072)] for a in (0, 1)},
    'base_fused': [s + (0,) for s in _blocks([16704], 768, 3072)],
    'large_fused': [s + (0,) for s in _blocks([8352], 1024, 4096)],
    'mini': [s + (1,) for s in _blocks([22], 128, 512)],
    **_gpu_test_lists(),
    'gpu_split': [(2000, 256, 512, 1), (1333, 96, 264, 0), (3000, 512, 256, 1)],
    'one_base_proj': [(16704, 768, 768, 0)],
    'one_problem_of_1000_tiles': [(200, 6400, 10240, 0), (100, 256, 256, 1)],
}


@pytest.fixture(scope='module', autouse=True)
def _library():
    import __graft_entry__ as ge
    if not os.path.exists(hip.LIB_PATH):
        ge.build()


@pytest.fixture(scope='module')
def plans(_library):
    return {name: hip.gemm_tn_multi_plan(shapes) for name, shapes in LISTS.items()}


@pytest.mark.parametrize('name', list(LISTS))
def test_query_equals_the_restated_rules(plans, name):
    got, want = plans[name], restate(LISTS[name])
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for field in ('q0', 'nq', 'problems', 'grid'):
            assert g[field] == w[field], (name, k, field)
        assert g['order'] == w['order'], (name, k)


def test_the_lists_are_the_cases_they_are_meant_to_be(plans):
    """What each list is there for, stated in numbers: a wrong list would make the comparison above vacuous."""
    def tiles(name):
        return [sum(p[0] for p in L['problems']) for L in plans[name]]

    def classes(name):
        return [sorted({p[2] for p in L['problems']}, reverse=True) for L in plans[name]]
    for a in (0, 1):
        n = f'base_two_experts_acc{a}'
        assert tiles(n) == [2 * (9 + 27 + 4 * 36)] and classes(n) == [[261, 197, 64]]
        assert {p[3:] for p in plans[n][0]['problems']} == {((ACCUM if a else STORE), 0)}
    assert tiles('base_fused') == [216] and classes('base_fused') == [[261]]
    assert tiles('large_fused') == [384]
    assert [p[1:3] for p in plans['mini'][0]['problems']] == [(1, 1)] * 8           # nk = 1: nk_min / 8 = 0, no split
    # 6 tiles, but the shortest reduction has 6 K-tiles: 6 / 8 = 0, no split (as on the parent of this plan's extraction)
    assert [p[1:] for p in plans['gpu_small'][0]['problems']] == [(1, 11, ACCUM, 0), (1, 6, STORE, 0), (1, 16, ACCUM, 0)]
    # 6 tiles and >= 21 K-tiles: two ragged halves, atomics, the non-accumulating output zeroed first
    assert [p[1:] for p in plans['gpu_split'][0]['problems']] == [(2, 16, ATOMIC, 0), (2, 11, ATOMIC, 1), (2, 24, ATOMIC, 0)]
    assert plans['one_base_proj'][0]['problems'] == [(9, 27, 10, ATOMIC, 1)]        # 28 asked, 27 of 10 K-tiles cover 261
    assert [L['nq'] for L in plans['gpu_19_problems']] == [16, 3]
    assert tiles('gpu_20x64_tiles') == [960, 320]
    assert [(L['q0'], L['nq']) for L in plans['one_problem_of_1000_tiles']] == [(0, 1), (1, 1)]
    assert plans['one_problem_of_1000_tiles'][0]['grid'] == 1000


@pytest.mark.parametrize('name', list(LISTS))
def test_placement_properties(plans, name):
    for L in plans[name]:
        order, probs = L['order'], L['problems']
        assert L['grid'] == len(order) and L['grid'] % 8 == 0 and L['grid'] <= 1024
        # every workgroup of every problem exactly once; everything else runs nothing
        want = Counter((q << 12) | l for q, p in enumerate(probs) for l in range(p[0] * p[1]))
        assert Counter(c for c in order if c != NOP) == want
        assert max(want.values()) == 1
        assert len(order) - sum(want.values()) == order.count(NOP)
        cols = [order[x::8] for x in range(8)]
        per_class = []
        for col in cols:
            work = [c for c in col if c != NOP]
            assert col == work + [NOP] * (len(col) - len(work))                     # idle workgroups come last
            costs = [probs[c >> 12][2] for c in work]
            assert costs == sorted(costs, reverse=True)                             # long reductions are dispatched first
            per_class.append(Counter(costs))
        for cost in {p[2] for p in probs}:                                          # every XCD gets the same mix
            counts = [c[cost] for c in per_class]
            assert max(counts) - min(counts) <= 1, (name, cost, counts)


@pytest.mark.parametrize('shapes, message', [
    ([(64, 256 * 33, 256 * 32, 0)], 'exceed one launch'),                           # 1 056 workgroups > 1 024
    ([(64, 256 * 65, 256 * 64, 0)], 'too many tiles'),                              # 4 160 tiles > 4 096
    ([(128, 256, 256, 1), (64, 256 * 33, 256 * 32, 0)], 'exceed one launch'),       # behind a launch that is fine
    ([(128, 256, 256, 1), (0, 256, 256, 1)], 'bad shape in problem 1'),
])
def test_a_call_that_cannot_be_planned_is_an_error(shapes, message):
    """The launcher raises the same error from the same plan before it enqueues anything (vlmo_gemm_tn_multi: plan,
    then VLMO_CHECK_ARG, then the first memset); tests/test_kernels_gpu.py checks that no output is touched."""
    if shapes[-1][0] > 0:
        with pytest.raises(PlanError, match=message):
            restate(shapes)
    with pytest.raises(RuntimeError, match=message):
        hip.gemm_tn_multi_plan(shapes)
