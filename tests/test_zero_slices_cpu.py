"""zero.ZeroAdam on slice tables, without a GPU: the harness of tests/zero_cases.py on ``EmuZero``, which restates the two
kernel calls in torch over the DEVICE launch table (``tab.dev_i`` / ``tab.dev_c``), so everything up to the kernels -- the
partition, the entry addresses, the chunking, the skip set, the groups, the norm exchange, the per-parameter counters -- is
checked here against the fp64 oracle on whole tensors.  The same cases run on the HIP kernels in test_zero_slices_gpu.py.

The second half plants one error at a time and requires the harness to notice each: a harness that passes everything
proves nothing."""
import pytest

from exploremultimodal_amd import mt
from exploremultimodal_amd.zero import ZeroAdam
from tests import zero_cases as zc

VARIANTS = zc.VARIANTS


def test_the_cases_hold_the_edges_they_claim():
    """Read off the real ``_entries``: starts 0, 4, 8 and 12 bytes off 16-byte alignment, a misaligned entry longer than a
    chunk, a one-element entry, neighbours in different groups; at W > 1 a slice boundary inside a parameter and
    parameters wholly outside a rank's slice."""
    sim = zc.Sim(1, 0, 'cpu')
    sim.step(0, zc.oracle_run(True, 1.0, None)[0])
    ent = sim.opt._entries()
    assert {e[0] % 16 for e in ent} == {0, 4, 8, 12}
    assert all(e[0] % 16 == e[1] % 16 == e[2] % 16 == e[3] % 16 for e in ent)
    assert any(e[0] % 16 and e[4] > mt.CHUNK for e in ent) and any(e[4] == 1 for e in ent)
    for pt in sim.opt.parts:        # neighbours inside a bucket are in different lr / weight-decay groups
        mine = [e for e in ent if pt.pflat.data_ptr() <= e[0] < pt.pflat.data_ptr() + 4 * pt.padded]
        assert len(mine) > 1 and all(a[5] != b[5] for a, b in zip(mine, mine[1:]))
    assert len(ent) == len(zc.SINK_SHAPES) + len(zc.HOOK_SHAPES) - 1           # all but the parameter without a gradient
    cut = outside = 0
    for w, r in zc.ranks((2, 3, 8)):
        sim = zc.Sim(w, r, 'cpu')
        sim.step(0, zc.oracle_run(True, 1.0, None)[0])
        ent = sim.opt._entries()
        cut += sum(e[4] < e[6].numel() for e in ent)
        outside += len(zc.SINK_SHAPES) + len(zc.HOOK_SHAPES) - 1 - len({id(e[6]) for e in ent})
        assert r == 0 or all(pt.lo > 0 for pt in sim.opt.parts)
    assert cut >= 8 and outside >= 8


@pytest.mark.parametrize('world,rank', zc.ranks())
def test_each_rank_matches_the_whole_tensor_oracle(world, rank):
    worst = zc.Sim(world, rank, 'cpu').run()
    assert set(worst) == {'norm', 'coef', 'p', 'm', 'v'}


@pytest.mark.parametrize('rank', range(3))
@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_variants_at_world_3(variant, rank):
    sim = zc.Sim(3, rank, 'cpu', **VARIANTS[variant])
    sim.run()
    if 'bad_step' in VARIANTS[variant]:
        # the skipped step counted: FusedAdam's rule (its host-side counters do not count skips back)
        assert set(sim.opt._pstep.values()) <= {zc.STEPS, zc.STEPS - 1}


# ------------------------------------------------------------------------------------------------ planted errors
def _entries_through(monkeypatch, fn):
    orig = ZeroAdam._entries
    monkeypatch.setattr(ZeroAdam, '_entries', lambda self: fn(self, orig(self)))


def _plant_grad_at_lo(mp):
    def fn(self, ent):
        out = []
        for e in ent:
            pt = next(pt for pt in self.parts
                      if pt.pflat.data_ptr() <= e[0] < pt.pflat.data_ptr() + 4 * pt.padded)
            lo = (e[0] - pt.pflat.data_ptr()) // 4
            out.append((e[0], pt.bucket.shard32.data_ptr() + 4 * lo) + e[2:])
        return out
    _entries_through(mp, fn)


def _plant_end(delta):
    def plant(mp):
        _entries_through(mp, lambda self, ent: [e[:4] + (e[4] + delta,) + e[5:] for e in ent])
    return plant


def _plant_had_ignored(mp):
    orig = ZeroAdam._entries

    def entries(self):
        saved = [(pt.bucket, pt.bucket.had) for pt in self.parts if pt.bucket.had is not None]
        for b, had in saved:
            b.had = [True] * len(had)
        try:
            return orig(self)
        finally:
            for b, had in saved:
                b.had = had
    mp.setattr(ZeroAdam, '_entries', entries)


def _plant_neighbour_group(mp):
    _entries_through(mp, lambda self, ent: [e[:5] + (ent[i - 1 if i else 1][5],) + e[6:] for i, e in enumerate(ent)])


def _plant_other_sq_dropped(mp):
    def all_reduce_now(self, t):
        self.reduces += 1
    mp.setattr(zc.StubReducer, 'all_reduce_now', all_reduce_now)


def _plant_one_bias_correction(mp):
    state = {'step': None}
    orig_step, orig_args = ZeroAdam.step, mt.adam_args

    def step(self, *a, **k):
        state['step'] = None
        return orig_step(self, *a, **k)

    def adam_args(betas, eps, bias_correction, s, adam_w_mode):
        if state['step'] is None:
            state['step'] = s
        return orig_args(betas, eps, bias_correction, state['step'], adam_w_mode)
    mp.setattr(ZeroAdam, 'step', step)
    mp.setattr(mt, 'adam_args', adam_args)


def _plant_late_second_chunk(mp):
    orig = mt.chunks

    def chunks(numel):
        ct, cs = orig(numel)
        return ct, [s + 1 if s else 0 for s in cs]
    mp.setattr(mt, 'chunks', chunks)


# name -> (how to plant it, the kinds of check (zero_cases.Broke) that must fire somewhere in the cases below).  An address
# outside the optimizer's buffers can only be caught by the table walk: neither the emulation nor a GPU may follow it.
PLANTED = {
    'gradient address taken at lo instead of lo - pt.lo': (_plant_grad_at_lo, {'table'}),
    'slice end one short': (_plant_end(-1), {'value'}),
    'slice end one long': (_plant_end(+1), {'table', 'untouched'}),
    'had skip set ignored': (_plant_had_ignored, {'untouched'}),
    "entry gets its neighbour's group": (_plant_neighbour_group, {'value'}),
    'other_sq dropped from the clip norm': (_plant_other_sq_dropped, {'norm'}),
    'one bias correction for entries whose counters differ': (_plant_one_bias_correction, {'value'}),
    'second chunk starts one element late': (_plant_late_second_chunk, {'table'}),
}


def _kinds_that_fire():
    """Every case of W = 1 and 3; only zero_cases.Broke counts, a plain assertion of the harness's set-up is an error."""
    kinds, where = set(), []
    for world, rank in zc.ranks((1, 3)):
        try:
            zc.Sim(world, rank, 'cpu').run()
        except zc.Broke as e:
            kinds |= e.kinds
            where.append((world, rank, str(e)[:160]))
    return kinds, where


@pytest.mark.parametrize('name', sorted(PLANTED))
def test_planted_error_breaks_an_assertion(name, monkeypatch):
    plant, expected = PLANTED[name]
    plant(monkeypatch)
    kinds, where = _kinds_that_fire()
    assert kinds, f'{name}: every case still passes'
    assert expected <= kinds, (name, 'expected', expected, 'fired', kinds, where[:3])


def test_a_late_chunk_also_shows_in_the_values(monkeypatch):
    """With the coverage check of the table walk turned off the same planted error reaches the value checks: the element
    at the chunk boundary is not updated."""
    _plant_late_second_chunk(monkeypatch)
    monkeypatch.setattr(zc.CheckedZero, 'check_cover', False)
    kinds, where = _kinds_that_fire()
    assert 'table' not in kinds and 'value' in kinds, (kinds, where[:3])


def test_nothing_planted_breaks_nothing():
    """Control of the control: the loop of the planted-error test, with nothing planted."""
    assert _kinds_that_fire() == (set(), [])
