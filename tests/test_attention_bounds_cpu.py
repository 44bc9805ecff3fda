"""The bounds of tests/attn_cases.py against the torch emulation of the attention kernels' arithmetic
(tests/attn_emul.py), without a GPU:

  1. the emulation stays inside every per-element bound, the lse tolerance and the earlier floors on every case of
     tests/test_attention_peaked_gpu.py, and every case keeps the premise it exists for;
  2. the lse tolerance is four times the emulation's worst error, for both forms of the forward;
  3. each planted error of attn_emul breaks a bound on the new cases; which of them the earlier floors let through on
     Gaussian inputs is printed (run with -s), and the two lazy-maximum ones must be among those."""
import pytest
import torch

from exploremultimodal_amd import hip
from tests import attn_cases as ac
from tests import attn_emul as em

DROP = hip.drop_params(0.1, True)
TABLE = dict(ac.case_table())


def _case(name=None, **kw):
    kw = kw or TABLE[name]
    case = ac.make_case(name or 'flat', 'cpu', **kw)
    keep = case.keep(ac.DROP_SEED, DROP[0]) if kw['drop'] else None
    inv_keep = DROP[1] if kw['drop'] else 1.0
    return case, keep, inv_keep


@pytest.mark.parametrize('name', list(TABLE))
def test_emulation_is_inside_every_bound(name):
    case, keep, inv_keep = _case(name)
    ref = ac.reference(case, keep, inv_keep)
    rec = ac.assert_premises(case, ref)
    print(f'{name}: premises {rec}')
    ac.assert_within(em.run(case, keep, inv_keep), ref, case)


def test_lse_tolerance_is_four_times_the_emulations_worst_error():
    """both forms of the forward on every case and on Gaussian inputs (the earlier tests compare lse at this tolerance
    too): the stale maximum of the lazy form costs nothing measurable"""
    worst = {}
    for name in list(TABLE) + ['flat']:
        case, keep, inv_keep = _case(name) if name in TABLE else _case(**OLD['l_norescale'])
        want = ac.reference(case, keep, inv_keep)['lse']
        ok = ~want.isnan()
        for form, fwd in (('lazy', em.fwd_lazy), ('exact', em.fwd_exact)):
            have = em.run(case, keep, inv_keep, forward=fwd)['lse'].double()
            err, mag = (have[ok] - want[ok]).abs(), want[ok].abs()
            assert bool((4 * err <= ac.lse_tol(want[ok])).all()), (name, form, (4 * err / ac.lse_tol(want[ok])).max().item())
            small = mag <= 8
            w = worst.setdefault(form, [0.0, 0.0, 0.0])
            w[0] = max(w[0], err[small].max().item() if small.any() else 0.0)
            w[1] = max(w[1], (err[~small] / mag[~small]).max().item() if (~small).any() else 0.0)
            w[2] = max(w[2], mag.max().item())
    for form, (a, b, m) in worst.items():
        print(f'lse, {form} form: worst error {a:.3g} at |lse| <= 8, {b:.3g} |lse| above, |lse| up to {m:.0f}')
    # the constants are what was measured, not something far above it
    assert ac.LSE_A <= 5 * max(w[0] for w in worst.values()) and ac.LSE_B <= 5 * max(w[1] for w in worst.values())


# planted error -> the new cases it must break a bound on
MUTATIONS = {
    'l_norescale': ('rise-261-h2-tail', 'rise-513-h1-tail'),
    'O_norescale': ('rise-261-h2-tail', 'rise-513-h1-tail'),
    'delta_neighbor': ('rise-261-h2-tail', 'mixed-289-h1-tile'),
    'lse_unit': ('rise-261-h2-tail', 'low-513-h2-tail'),
    'kbias9': ('spike-261_261_261-h1-none',),
    'dropmask9': ('rise-261-h2-tail-drop', 'mixed-289-h1-tile-drop'),
    'no_inv_keep_dv': ('rise-261-h2-tail-drop', 'mixed-513-h1-tile-drop'),
}
# the earlier tests' kind of input (tests/kernel_refs._attn_case): N(0, 1) operands, a masked tail, with dropout for the
# mutations that need it
OLD = {m: dict(pattern='flat', lens=(197, 261), heads=2, mask='tail', drop=m in ('dropmask9', 'no_inv_keep_dv'), seed=5)
       for m in MUTATIONS}
OLD['kbias9'] = dict(pattern='flat', lens=(261, 261), heads=2, mask='tile', drop=False, seed=5)   # keys 254 .. 258 masked


@pytest.mark.parametrize('mut', list(MUTATIONS))
def test_planted_error_breaks_a_bound_on_the_new_cases(mut):
    for name in MUTATIONS[mut]:
        case, keep, inv_keep = _case(name)
        ref = ac.reference(case, keep, inv_keep)
        r = ac.ratios(em.run(case, keep, inv_keep, mut=(mut,)), ref, case)
        broken = {k: round(v, 2) for k, v in r.items() if not v <= 1.0}
        print(f'{mut} on {name}: error / bound ' + ' '.join(f'{k} {v:.3g}' for k, v in r.items()))
        assert broken, f'{mut} passes every bound on {name}'
    case, keep, inv_keep = _case(**OLD[mut])
    ref = ac.reference(case, keep, inv_keep)
    clean = ac.floors(em.run(case, keep, inv_keep), ref, case)
    assert all(v <= 1.0 for v in clean.values()), clean
    f = ac.floors(em.run(case, keep, inv_keep, mut=(mut,)), ref, case)
    missed = all(v <= 1.0 for v in f.values())
    print(f'{mut} on Gaussian inputs under the earlier floors (ctx, dqkv, qv; lse was never compared): '
          f'{"MISSED" if missed else "caught"} ' + ' '.join(f'{k} {v:.3g}' for k, v in f.items()))
    if mut in ('l_norescale', 'O_norescale'):
        assert missed, 'the lazy rescale is taken on Gaussian inputs after all'
        counts = [ac.lazy_rescales(h['S'], h['S'].shape[0])[0] for h in ref['heads']]
        assert max(max(c) for c in counts) == 0


@pytest.mark.parametrize('n', [261, 289, 513])
def test_one_live_key_on_the_emulation(n):
    case = ac.one_live_key_case(n, 'cpu')
    ac.check_one_live_key(em.run(case), ac.reference(case), case)


def test_uniform_on_the_emulation():
    case = ac.uniform_case('cpu')
    ac.check_uniform(em.run(case), ac.reference(case), case)


def test_lazy_rescales_of_rise_at_261_tokens():
    """the issue's figure: at least 8 predicted rescales after the first in some wave (all nine waves take 8)"""
    case, _, _ = _case('rise-261-h2-tail')
    ref = ac.reference(case)
    counts = [ac.lazy_rescales(h['S'], 261)[0] for h in ref['heads']]
    print('rise, N = 261: rescales per wave', counts)
    assert all(max(c) >= 8 for c in counts)
