"""The result record's layout is fixed: restarts._pack reproduces, for 33 combinations of the optional sections (the 20
valid ones of the first five sections; each of the six later sections alone, all together, and all but one), the vectors
the commit before the table of optional outputs packed (tests/golden/record_layout.npz, written by tests/record_layout.py),
and restarts._unpack returns every key and value that went in."""
import numpy as np
import pytest

from remixt_amd import posteriors, sampling

from . import record_layout as rl


@pytest.fixture(scope='module')
def golden():
    return np.load(rl.GOLDEN)


@pytest.fixture(scope='module')
def result():
    return rl.synthetic_result()


def test_all_valid_combinations_are_stored(golden):
    assert len(rl.early_combos()) == 20 and len(set(rl.early_combos())) == 20
    assert len(rl.combos()) == 33 and len(set(rl.combos())) == 33 and len(set(rl.combo_key(c) for c in rl.combos())) == 33
    assert rl.combos()[:20] == rl.early_combos()
    assert sorted(golden.files) == sorted(rl.combo_key(c) + s for c in rl.combos() for s in ('_f', '_i8'))


def test_later_combinations_cover_each_section_alone_all_and_all_but_one():
    later = [c[5:] for c in rl.later_combos()]
    n = len(rl.LATER)
    ext, ln = rl.LATER.index('ext'), rl.LATER.index('len')
    for i, k in enumerate(rl.LATER):
        alone = [j == i or (k == 'len' and j == ext) for j in range(n)]
        assert later[i] == tuple(alone), k
        assert rl.later_combos()[i][:5] == (False, False, k in ('mom', 'calls', 'extr'), 0, False)
        but = [j != i and not (k == 'ext' and j == ln) for j in range(n)]
        assert later[n + 1 + i] == tuple(but), k
    assert later[n] == (True,) * n
    assert all(c[:5] == (True, True, True, rl.BINS, True) for c in rl.later_combos()[n:])


def test_every_value_of_the_full_record_is_distinct(golden):
    f = golden[rl.combo_key(rl.later_combos()[len(rl.LATER)]) + '_f']
    assert len(f) == 527 and len(set(f.tolist())) == 527


@pytest.mark.parametrize('combo', rl.combos(), ids=rl.combo_key)
def test_pack_reproduces_the_stored_record(golden, result, combo):
    f, i8 = rl.pack(result, combo)
    gf, gi = golden[rl.combo_key(combo) + '_f'], golden[rl.combo_key(combo) + '_i8']
    assert f.dtype == gf.dtype and i8.dtype == gi.dtype
    assert np.array_equal(f, gf) and np.array_equal(i8, gi)


@pytest.mark.parametrize('combo', rl.combos(), ids=rl.combo_key)
def test_unpack_returns_what_went_in(golden, result, combo):
    smp, post, reg, bins, call, mom, ext, ln, brk, calls, extr = combo
    out = rl.unpack(golden[rl.combo_key(combo) + '_f'], golden[rl.combo_key(combo) + '_i8'], combo)
    arrays = ['h', 'cn', 'p_outlier_total', 'p_outlier_allele', 'total_likelihood_mask', 'allele_likelihood_mask']
    stats = ['elbo', 'elbo_diff', 'ploidy', 'proportion_divergent', 'error_message'] + rl.PARAM_NAMES
    groups = []
    if smp:
        arrays += ['cn_sample_agreement', 'cn_state_agreement']; stats += list(sampling.SUMMARY_STATS)
    if post:
        arrays += list(posteriors.COMPACT_ARRAYS); stats += list(posteriors.SUMMARY_STATS)
    if reg:
        groups.append(('region_events', posteriors.REGION_ARRAYS, ['names']))
    if bins:
        groups.append(('region_change_counts', posteriors.COUNT_ARRAYS, ['names', 'bins']))
    if call:
        groups.append(('call_confidence', posteriors.CALL_ARRAYS, ['names'])); stats.append('cn_logprob')
    if mom:
        groups.append(('region_cn_moments', posteriors.MOMENT_ARRAYS, ['names'])); stats += list(posteriors.MOMENT_STATS)
    if ext:
        groups.append(('event_extents', posteriors.EXTENT_ARRAYS, ['names']))
    if ln:
        groups.append(('event_lengths', posteriors.SPAN_ARRAYS + posteriors.SPAN_EDGE_ARRAYS, ['names']))
    if brk:
        arrays += list(posteriors.BREAKEND_ARRAYS)
    if calls:
        groups.append(('region_calls', posteriors.REGION_CALL_ARRAYS, ['names']))
    if extr:
        groups.append(('region_cn_extremes', posteriors.EXTREME_ARRAYS, ['names', 'bins']))
    assert set(out) == set(arrays) | set(g[0] for g in groups) | {'brk_cn', 'stats'}
    for k in arrays:
        assert np.array_equal(out[k], result[k]) and np.shape(out[k]) == np.shape(result[k]), k
    assert list(out['brk_cn']) == rl.BRK_IDS
    for k in rl.BRK_IDS:
        assert np.array_equal(out['brk_cn'][k], result['brk_cn'][k])
    assert set(out['stats']) == set(stats) | {'num_clones', 'num_segments', 'mode_idx', 'divergence_weight'}
    for k in stats:
        assert out['stats'][k] == result['stats'][k], k
    assert (out['stats']['num_clones'], out['stats']['num_segments']) == (rl.M, rl.N)
    assert out['stats']['mode_idx'] == rl.INIT_PARAMS['mode_idx'] and out['stats']['divergence_weight'] == rl.INIT_PARAMS['divergence_weight']
    for name, keys, plain in groups:
        assert set(out[name]) == set(keys) | set(plain)
        for k in plain:
            assert out[name][k] == result[name][k]
        for k in keys:
            want = result[name][k]
            if out[name][k].dtype == bool:      # a flag: the record carries it as a float and hands it back as a flag
                assert k.endswith('censored'), (name, k)
                want = want != 0
            assert np.array_equal(out[name][k], want) and np.shape(out[name][k]) == np.shape(want), (name, k)
    if ext:
        assert all(out['event_extents'][k].dtype == (float if k == 'p_event' else (bool if k.endswith('_censored') else np.int64))
                   for k in posteriors.EXTENT_ARRAYS)


def test_flags_come_back_with_both_values(result):
    """The stored records hold distinct whole numbers in the flags, which all come back True: here 0 and 1, as a fit sets them."""
    combo = rl.later_combos()[len(rl.LATER)]      # everything on
    res = dict(result, event_extents=dict(result['event_extents']), event_lengths=dict(result['event_lengths']))
    flags = {'left_censored': [False, True], 'right_censored': [True, False]}
    res['event_extents'].update((k, np.array(v)) for k, v in flags.items())
    res['event_lengths']['length_censored'] = np.array([True, False])
    out = rl.unpack(*rl.pack(res, combo), combo)
    for k, v in flags.items():
        assert out['event_extents'][k].dtype == bool and out['event_extents'][k].tolist() == v, k
    assert out['event_lengths']['length_censored'].dtype == bool and out['event_lengths']['length_censored'].tolist() == [True, False]
    for k in posteriors.EXTENT_ARRAYS[:-2]:
        assert np.array_equal(out['event_extents'][k], result['event_extents'][k]), k
