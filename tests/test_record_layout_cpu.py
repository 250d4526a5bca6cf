"""The result record's layout is fixed: restarts._pack reproduces, for all 20 valid combinations of the optional sections,
the vectors the commit before restarts._record_sections packed (tests/golden/record_layout.npz, written by
tests/record_layout.py), and restarts._unpack returns every key and value that went in."""
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
    assert len(rl.combos()) == 20 and len(set(rl.combos())) == 20
    assert sorted(golden.files) == sorted(rl.combo_key(c) + s for c in rl.combos() for s in ('_f', '_i8'))


@pytest.mark.parametrize('combo', rl.combos(), ids=rl.combo_key)
def test_pack_reproduces_the_stored_record(golden, result, combo):
    f, i8 = rl.pack(result, combo)
    gf, gi = golden[rl.combo_key(combo) + '_f'], golden[rl.combo_key(combo) + '_i8']
    assert f.dtype == gf.dtype and i8.dtype == gi.dtype
    assert np.array_equal(f, gf) and np.array_equal(i8, gi)


@pytest.mark.parametrize('combo', rl.combos(), ids=rl.combo_key)
def test_unpack_returns_what_went_in(golden, result, combo):
    smp, post, reg, bins, call = combo
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
            assert np.array_equal(out[name][k], result[name][k]) and np.shape(out[name][k]) == np.shape(result[name][k]), (name, k)
