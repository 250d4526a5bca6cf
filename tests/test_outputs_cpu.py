"""The table of optional fit outputs (remixt_amd/outputs.py): what `resolve` makes of a config against the single
posteriors.*_on checks and their messages, that every entry point refuses a bad config before it builds a model, the
store keys and shapes of a result with every output on (recorded from the commit before the table), and the two helpers
of the restart classes' fan-out."""
import numpy as np
import pytest

from remixt_amd import outputs, posteriors, restarts, sampling, synthetic
from remixt_amd.analysis import pipeline

REGIONS = [('arm', 0, 9), ('gene', 3, 4), ('one', 7, 7)]
EXTENTS = [('e0', 3, 'loh'), ('e1', 8, ('hdel', None))]


# ---- resolve ----------------------------------------------------------------------------------------------------------
def _expected(config, n=None):
    """What the single checks of posteriors make of `config`, by output name."""
    from remixt_amd import defaults
    get = lambda k: defaults.get_param(config, k)
    return {'samples': (get('num_cn_samples'), get('cn_sample_seed')) if get('num_cn_samples') > 0 else None,
            'posterior_summary': True if get('cn_posterior_summary') else None,
            'region_events': None if get('cn_regions') is None else posteriors.parse_regions(get('cn_regions')),
            'change_counts': posteriors.change_bins(config) or None,
            'call_confidence': posteriors.call_confidence_on(config) or None,
            'region_moments': posteriors.region_moments_on(config) or None,
            'event_extents': posteriors.extents_on(config, n),
            'event_lengths': posteriors.lengths_on(config, n),
            'breakend_changes': True if get('cn_breakend_changes') else None,
            'region_calls': posteriors.region_calls_on(config) or None,
            'region_extremes': posteriors.region_extremes_on(config) or None}


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return type(a) is type(b) and a == b


GOOD = [
    {},
    {'num_cn_samples': 0, 'cn_posterior_summary': False, 'cn_regions': None, 'cn_region_change_bins': 0, 'cn_call_confidence': False,
     'cn_region_moments': False, 'cn_event_extents': None, 'cn_event_lengths': False, 'cn_breakend_changes': False, 'cn_region_calls': False,
     'cn_region_extremes': False},
    {'num_cn_samples': 7, 'cn_sample_seed': 3},
    {'cn_posterior_summary': True},
    {'cn_regions': REGIONS},
    {'cn_regions': REGIONS, 'cn_region_change_bins': 1},
    {'cn_regions': REGIONS, 'cn_region_change_bins': 16},
    {'cn_regions': REGIONS, 'cn_call_confidence': True},
    {'cn_regions': REGIONS, 'cn_region_moments': True},
    {'cn_regions': REGIONS, 'cn_region_calls': True},
    {'cn_regions': REGIONS, 'cn_region_extremes': True},
    {'cn_event_extents': EXTENTS},
    {'cn_event_extents': EXTENTS, 'cn_extent_window': (5, 9)},
    {'cn_event_extents': EXTENTS, 'cn_event_lengths': True},
    {'cn_event_extents': EXTENTS, 'cn_event_lengths': True, 'cn_event_length_edges': [1e4, 1e6], 'cn_extent_window': 100},
    {'cn_event_length_edges': [-1.]},      # (not looked at while cn_event_lengths is off)
    {'cn_breakend_changes': True},
    {'num_cn_samples': 2, 'cn_posterior_summary': True, 'cn_regions': REGIONS, 'cn_region_change_bins': 4, 'cn_call_confidence': True,
     'cn_region_moments': True, 'cn_event_extents': EXTENTS, 'cn_event_lengths': True, 'cn_event_length_edges': (5e5,), 'cn_breakend_changes': True,
     'cn_region_calls': True, 'cn_region_extremes': True},
]

# (config, the message of the commit before the table, word for word)
BAD = [
    ({'cn_region_change_bins': 4}, 'cn_region_change_bins needs cn_regions'),
    ({'cn_regions': REGIONS, 'cn_region_change_bins': 17}, 'cn_region_change_bins must be in 0 .. 16'),
    ({'cn_regions': REGIONS, 'cn_region_change_bins': -1}, 'cn_region_change_bins must be in 0 .. 16'),
    ({'cn_call_confidence': True}, 'cn_call_confidence needs cn_regions'),
    ({'cn_region_moments': True}, 'cn_region_moments needs cn_regions'),
    ({'cn_region_calls': True}, 'cn_region_calls needs cn_regions'),
    ({'cn_region_extremes': True}, 'cn_region_extremes needs cn_regions'),
    ({'cn_event_extents': [('e0', 3)]}, "cn_event_extents: an entry is (name, segment, event), not ('e0', 3)"),
    ({'cn_event_extents': [('e0', -1, 'loh')]}, "cn_event_extents: the segment of 'e0' must be an index >= 0"),
    ({'cn_event_extents': [('e0', 20, 'loh')]}, 'cn_event_extents: a segment is outside the experiment'),
    ({'cn_event_extents': EXTENTS, 'cn_extent_window': 2048}, 'a window needs widths >= 0 and at most 4096 slots'),
    ({'cn_event_lengths': True}, 'cn_event_lengths needs cn_event_extents'),
    ({'cn_event_extents': EXTENTS, 'cn_event_lengths': True, 'cn_extent_window': 128},
     'cn_event_lengths: cn_extent_window (128, 128) gives a table of more than 16384 entries'),
    ({'cn_event_extents': EXTENTS, 'cn_event_lengths': True, 'cn_event_length_edges': 5}, 'cn_event_length_edges: a list of lengths'),
    ({'cn_event_extents': EXTENTS, 'cn_event_lengths': True, 'cn_event_length_edges': [1e4, 0.]}, 'cn_event_length_edges: every length must be > 0'),
    ({'cn_event_extents': EXTENTS, 'cn_event_lengths': True, 'cn_event_length_edges': [float('inf')]}, 'cn_event_length_edges: every length must be > 0'),
]


def test_table():
    assert [o.name for o in outputs.OUTPUTS] == ['samples', 'posterior_summary', 'region_events', 'change_counts', 'call_confidence', 'region_moments',
                                                 'event_extents', 'event_lengths', 'breakend_changes', 'region_calls', 'region_extremes']
    assert [o.switch for o in outputs.OUTPUTS] == ['cn_samples', 'cn_posterior', 'region_names', 'change_bins', 'call_confidence', 'cn_moments',
                                                   'extent_names', 'length_edges', 'breakend_changes', 'region_calls', 'region_extremes']
    from remixt_amd import defaults
    keys = [k for o in outputs.OUTPUTS for k in o.keys]
    assert len(keys) == len(set(keys)) == len(outputs.CONFIG_KEYS) and all(hasattr(defaults, k) for k in keys)


@pytest.mark.parametrize('config', GOOD, ids=lambda c: '+'.join(sorted(c)) or 'defaults')
@pytest.mark.parametrize('n', [None, 20])
def test_resolve_returns_what_the_single_checks_return(config, n):
    sel = outputs.resolve(config, n)
    want = _expected(config, n)
    assert list(sel) == [o.name for o in outputs.OUTPUTS]
    for name in want:
        assert _same(sel[name], want[name]), (name, sel[name], want[name])
    # the record switches, as fit_restarts_distributed spelled them before the table
    sw = sel.record_switches()
    names = None if want['region_events'] is None else [str(r[0]) for r in config['cn_regions']]
    assert sw == dict(cn_samples=want['samples'] is not None, cn_posterior=want['posterior_summary'] is not None, region_names=names,
                      change_bins=want['change_counts'] or 0, call_confidence=want['call_confidence'] is not None,
                      cn_moments=want['region_moments'] is not None,
                      extent_names=None if want['event_extents'] is None else want['event_extents'][0],
                      length_edges=None if want['event_lengths'] is None else len(want['event_lengths'][4]),
                      breakend_changes=want['breakend_changes'] is not None, region_calls=want['region_calls'] is not None,
                      region_extremes=want['region_extremes'] is not None)


@pytest.mark.parametrize('config,message', BAD, ids=[m[:48] + '|' + '+'.join(sorted(c)) for c, m in BAD])
def test_bad_configs_fail_with_the_same_words_before_any_model(config, message, monkeypatch):
    with pytest.raises(ValueError) as err:
        outputs.resolve(config, 20)
    assert str(err.value) == message

    def no_model(*args, **kwargs):
        raise AssertionError('a model was built before the config was checked')
    monkeypatch.setattr(restarts, 'BreakpointModel', no_model)
    monkeypatch.setattr(pipeline, 'BreakpointModel', no_model)
    e = synthetic.make_experiment(20, num_clones=3, max_copy_number=3, num_chains=2, seed=0)
    ps = synthetic.make_init_params(e, 2, 3)
    for call in (lambda: pipeline.fit(e, ps[0], config), lambda: pipeline.fit_restarts(e, dict(enumerate(ps)), config),
                 lambda: restarts.fit_restarts_distributed(e, ps, 3, **config)):
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == message


def test_distributed_keywords_that_are_no_config_keys_stay_model_kwargs(monkeypatch):
    seen = {}

    class Stop(Exception):
        pass

    def groups(experiment, init_params, max_copy_number, **kwargs):
        seen.update(kwargs)
        raise Stop()
    monkeypatch.setattr(restarts, 'RestartGroups', groups)
    e = synthetic.make_experiment(20, num_clones=3, max_copy_number=3, num_chains=2, seed=0)
    ps = synthetic.make_init_params(e, 2, 3)
    with pytest.raises(Stop):
        restarts.fit_restarts_distributed(e, ps, 3, cn_regions=REGIONS, cn_region_calls=True, num_cn_samples=2, normal_contamination=False, do_h_update=False)
    assert seen['normal_contamination'] is False and seen['do_h_update'] is False
    assert not (set(seen) & set(outputs.CONFIG_KEYS))


# ---- store ------------------------------------------------------------------------------------------------------------
def _fake_result(e, rng, M=3):
    N = len(e.x)
    res = {'h': np.array([0.1, 0.2, 0.3]), 'cn': np.ones((N, M, 2), dtype=int),
           'brk_cn': dict((k, rng.randint(0, 3, size=M)) for k in e.breakpoints),
           'p_outlier_total': rng.uniform(size=(N, 2)), 'p_outlier_allele': rng.uniform(size=(N, 2)),
           'total_likelihood_mask': rng.randint(0, 2, size=N), 'allele_likelihood_mask': rng.randint(0, 2, size=N)}
    res['stats'] = {'elbo': -1234.5 - rng.uniform(), 'elbo_diff': 0.25, 'ploidy': 2.7, 'proportion_divergent': 0.1, 'error_message': '',
                    'negbin_r_0': 1., 'negbin_r_1': 2., 'betabin_M_0': 3., 'betabin_M_1': 4.}
    return res


def _full_result(e, rng, M=3):
    """Every optional output on, each added as a fit adds it."""
    res = _fake_result(e, rng, M)
    N, K = len(e.x), len(e.breakpoints)
    names, bins, edges = [r[0] for r in REGIONS], 4, 3
    R, A, B = len(names), len(EXTENTS), posteriors.EXTREME_BINS
    sampling.add_sample_summary(res, rng.randint(0, 3, size=(4, N, M, 2)), e.l)
    summary = dict((k, rng.uniform(size=(N, M) if k.startswith('total_cn') else (N,))) for k in posteriors.COMPACT_ARRAYS)
    summary['expected_alleles_subclonal'] = rng.uniform(0, 2, size=N)
    posteriors.add_posterior_summary(res, summary, e.l)
    posteriors.add_region_events(res, names, dict((k, rng.uniform(size=R)) for k in posteriors.REGION_ARRAYS))
    posteriors.add_region_change_counts(res, names, bins, dict((k, rng.dirichlet(np.ones(bins), size=R)) for k in posteriors.COUNT_ARRAYS))
    posteriors.add_call_confidence(res, names, dict((k, rng.uniform(size=R)) for k in posteriors.CALL_ARRAYS), -3.)
    shapes = posteriors.moment_shapes(R, M)
    posteriors.add_region_cn_moments(res, names, dict((k, rng.uniform(size=shapes[k])) for k in posteriors.MOMENT_ARRAYS), (0.5, 0.25))
    posteriors.add_event_extents(res, [x[0] for x in EXTENTS], dict((k, rng.randint(0, 9, size=A)) for k in posteriors.EXTENT_ARRAYS))
    posteriors.add_event_lengths(res, [x[0] for x in EXTENTS], dict([(k, rng.uniform(size=A)) for k in posteriors.SPAN_ARRAYS] +
                                                                   [(k, rng.uniform(size=(A, edges))) for k in posteriors.SPAN_EDGE_ARRAYS]))
    posteriors.add_breakend_changes(res, dict((k, rng.uniform(size=(K, 2) if k == 'p_change' else (K,))) for k in posteriors.BREAKEND_ARRAYS))
    posteriors.add_region_calls(res, names, dict((k, rng.uniform(size=R)) for k in posteriors.REGION_CALL_ARRAYS))
    posteriors.add_region_cn_extremes(res, names, dict((k, rng.dirichlet(np.ones(B), size=(R, M - 1))) for k in posteriors.EXTREME_ARRAYS))
    return res


REFERENCE_KEYS = ['/h', '/cn', '/mix', '/brk_cn']
# solution keys in the order written, with their shapes, for N = 40 segments, M = 3, K = 1 breakpoint, 3 regions, 4 count bins,
# 2 extent entries and 3 length edges: as the commit before the table of outputs wrote them
OPTIONAL_KEYS = [
    ('/cn_sample_agreement', (40, 3)), ('/cn_state_agreement', (40,)),
    ('/cn_posterior_prob', (40,)), ('/cn_posterior_max', (40,)), ('/cn_posterior_entropy', (40,)), ('/p_subclonal', (40,)), ('/p_loh', (40,)),
    ('/p_hdel', (40,)), ('/total_cn_mean', (40, 3)), ('/total_cn_sd', (40, 3)),
    ('/region_names', (3,)), ('/p_all_loh', (3,)), ('/p_any_loh', (3,)), ('/p_all_hdel', (3,)), ('/p_any_hdel', (3,)), ('/p_any_subclonal', (3,)),
    ('/p_no_change', (3,)), ('/p_no_total_change', (3,)),
    ('/num_changes', (3, 4)), ('/num_total_changes', (3, 4)),
    ('/p_call', (3,)), ('/p_call_unphased', (3,)), ('/p_call_total', (3,)),
    ('/region_length', (3,)), ('/region_total_cn_mean', (3, 3)), ('/region_total_cn_cov', (3, 9)), ('/region_fraction_mean', (3, 4)),
    ('/region_fraction_cov', (3, 16)),
    ('/extent_names', (2,)), ('/extent_p_event', (2,)), ('/extent_left_q05', (2,)), ('/extent_left_q50', (2,)), ('/extent_left_q95', (2,)),
    ('/extent_right_q05', (2,)), ('/extent_right_q50', (2,)), ('/extent_right_q95', (2,)), ('/extent_left_censored', (2,)),
    ('/extent_right_censored', (2,)),
    ('/span_names', (2,)), ('/span_length_q05', (2,)), ('/span_length_q50', (2,)), ('/span_length_q95', (2,)), ('/span_length_censored', (2,)),
    ('/span_p_length_le', (2, 3)), ('/span_p_length_undetermined', (2, 3)),
    ('/region_call_log_prob', (3,)), ('/region_call_log_prob_call', (3,)), ('/region_call_n_differ', (3,)),
    ('/region_peak_total_pmf', (3, 32)), ('/region_floor_total_pmf', (3, 32)),
    ('/breakend_p_change', (1, 2)), ('/breakend_p_change_both', (1,)), ('/breakend_p_change_neither', (1,)), ('/breakend_p_change_only_first', (1,)),
    ('/breakend_p_change_only_second', (1,)),
]


class _OrderedStore(pipeline._Store):
    """pipeline._Store, remembering the order of the writes."""

    def __init__(self, *args):
        pipeline._Store.__init__(self, *args)
        self.order = []

    def __setitem__(self, k, v):
        self.order.append((self._key(k), tuple(v.shape)))
        pipeline._Store.__setitem__(self, k, v)


def _collate(tmp_path, tag, results, e):
    with _OrderedStore(str(tmp_path / (tag + '.store')), 'w') as store:
        best = pipeline.collate_results(store, e, results, {})
        return best, store.order, set(store._key(k) for k in store.keys())


def test_store_keys_and_shapes(tmp_path):
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=4, num_chains=3, seed=2)
    assert (len(e.x), len(e.breakpoints)) == (40, 1)
    rng = np.random.RandomState(0)
    off = {0: _fake_result(e, rng), 3: _fake_result(e, rng)}
    on = {0: _full_result(e, rng), 3: _full_result(e, rng)}
    top = ['/stats'] + ['/solutions/solution_%d%s' % (i, k) for i in (0, 3) for k in REFERENCE_KEYS] + ['/cn', '/mix', '/brk_cn']
    best, order, keys = _collate(tmp_path, 'off', off, e)
    assert best in off and [k for k, _ in order] == top and keys == set(top)
    best, order, keys = _collate(tmp_path, 'on', on, e)
    assert best in on
    fixed = dict((k, s) for k, s in order if k.endswith(tuple(REFERENCE_KEYS)) and k.startswith('/solutions/solution_0'))
    want = [('/stats', order[0][1])]
    for i in (0, 3):
        want += [('/solutions/solution_%d%s' % (i, k), fixed['/solutions/solution_0' + k]) for k in REFERENCE_KEYS]
        want += [('/solutions/solution_%d%s' % (i, k), s) for k, s in OPTIONAL_KEYS]
    want += [(k, fixed['/solutions/solution_0' + k]) for k in ('/cn', '/mix', '/brk_cn')]
    assert order == want
    assert keys == set(k for k, _ in want) and len(keys) == len(want)
    assert fixed['/solutions/solution_0/h'] == (3,) and fixed['/solutions/solution_0/mix'] == (3,) and fixed['/solutions/solution_0/cn'][0] == 40


# ---- the fan-out helpers of RestartGroups / DatasetGroups ---------------------------------------------------------------
def test_join_dict_with_shared_keys():
    parts = [{'length': np.array([5., 7.]), 'mean': np.arange(6.).reshape(3, 2)}, {'length': np.array([5., 7.]), 'mean': 10 + np.arange(4.).reshape(2, 2)}]
    out = restarts._join(parts, shared=('length',))
    assert list(out) == ['length', 'mean'] and out['length'] is parts[0]['length']
    assert np.array_equal(out['mean'], np.concatenate([parts[0]['mean'], parts[1]['mean']])) and out['mean'].shape == (5, 2)
    ext = [{'bins': 16, 'first_level': 0, 'peak_pmf': np.zeros((1, 2, 16))}, {'bins': 16, 'first_level': 0, 'peak_pmf': np.ones((3, 2, 16))}]
    out = restarts._join(ext, shared=('bins', 'first_level'))
    assert out['bins'] == 16 and out['first_level'] == 0 and out['peak_pmf'].shape == (4, 2, 16) and out['peak_pmf'][:, 0, 0].tolist() == [0, 1, 1, 1]
    one = restarts._join(parts[:1])
    assert np.array_equal(one['mean'], parts[0]['mean']) and np.array_equal(one['length'], parts[0]['length'])


def test_join_lists():
    assert restarts._join([[1, 2], [3], []]) == [1, 2, 3]
    a, b, c = np.zeros(2), np.ones(2), np.full(2, 2.)
    out = restarts._join([[a, b], [c]])
    assert len(out) == 3 and out[0] is a and out[2] is c


def test_join_lists_inside_a_dict():
    # p_parts of event_joint: per pattern an array (restarts, parts); cn of region_call: per restart a list over regions
    parts = [{'p_joint': np.zeros((2, 3)), 'p_parts': [np.zeros((2, 2)), np.zeros((2, 4))]},
             {'p_joint': np.ones((1, 3)), 'p_parts': [np.ones((1, 2)), np.ones((1, 4))]}]
    out = restarts._join(parts, each=('p_parts',))
    assert out['p_joint'].shape == (3, 3) and [p.shape for p in out['p_parts']] == [(3, 2), (3, 4)]
    assert out['p_parts'][1][:, 0].tolist() == [0, 0, 1]
    calls = [{'log_prob': np.zeros((2, 1)), 'cn': [['r0'], ['r1']]}, {'log_prob': np.ones((1, 1)), 'cn': [['r2']]}]
    out = restarts._join(calls, extend=('cn',))
    assert out['cn'] == [['r0'], ['r1'], ['r2']] and out['log_prob'].shape == (3, 1)


def test_per_group_slices_of_a_per_restart_argument():
    class G(object):
        slices = [slice((7 * g) // 3, (7 * (g + 1)) // 3) for g in range(3)]
        sets = ['a', 'b', 'c']
    cn = list('0123456')
    got = [restarts.RestartGroups._own(G, rs, cn) for rs in G.sets]
    assert got == [['0', '1'], ['2', '3'], ['4', '5', '6']] and sum(got, []) == cn
    assert [restarts.RestartGroups._own(G, rs, None) for rs in G.sets] == [None, None, None]
    arr = np.arange(14).reshape(7, 2)
    assert np.array_equal(np.concatenate([restarts.RestartGroups._own(G, rs, arr) for rs in G.sets]), arr)
