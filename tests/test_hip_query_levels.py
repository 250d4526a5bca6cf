"""The posterior queries at their four class levels on the device, driven by the table of remixt_amd/queries.py: every level
against the call it should forward to, bit for bit.
  model     rs.models[r].<query>(...)  ==  posteriors.batch_*(batch, r, 1, ...) with the restart axis stripped
  set       rs.<query>(...)            ==  posteriors.batch_*(batch, 0, R, ...)
  groups    RestartGroups.<query>(...) ==  the join of its sets' own answers
  datasets  DatasetGroups.<query>(...) ==  the list of its parts' answers
One fit per class: 40 segments in 3 chains, 3 clones, 4 restarts, two sweeps, fb_nv pinned so that the grouping picks no other
workgroup shape.  The regions: inside a chain, across a chain end, a single segment, the whole genome."""
import inspect

import numpy as np
import pytest

from remixt_amd import posteriors, queries, restarts, synthetic

pytestmark = pytest.mark.gpu

MAX_CN, R = 4, 4
REGIONS = [(2, 7), (10, 30), (17, 17), (0, 39)]
PATTERNS = [[(2, 4, 'loh'), (6, 7, 'not_loh')], [(10, 30, 'total')], [(17, 17, 'loh'), (0, 1, 'state'), (35, 39, 'not_hdel')]]
EXAMPLES = {
    'posterior_summary': [dict(), dict(marginals=True)],
    'region_events': [dict(regions=REGIONS)],
    'region_change_counts': [dict(regions=REGIONS), dict(regions=REGIONS, bins=5)],
    'region_cn_extremes': [dict(regions=REGIONS), dict(regions=REGIONS, quantity='minor', clone=2, bins=6, first_level=1)],
    'region_clone_extremes': [dict(regions=REGIONS, bins=8)],
    'region_cn_moments': [dict(regions=REGIONS)],
    'event_extent': [dict(anchors=[3, 17, 39], event='loh', window=6), dict(anchors=[12], event=('not_hdel', 'total'), window=(2, 9))],
    'conditional_summary': [dict(regions=REGIONS[:3], event='loh'), dict(regions=REGIONS, event=(None, 'total'), window=3)],
    'event_span': [dict(anchors=[3, 17], event='state', window=5), dict(anchors=[39], event='loh', window=(4, 0))],
    'event_joint': [dict(patterns=PATTERNS)],
    'focal_events': [dict(regions=REGIONS[:3]), dict(regions=REGIONS, flank=2)],
    'breakend_changes': [dict(arrays=True), dict()],
    'region_call': [dict(regions=REGIONS), dict(regions=REGIONS[:3], event=('not_loh', None))],
    'region_alternatives': [dict(regions=REGIONS), dict(regions=REGIONS[:3], k=3, event=(None, 'total'))],
    'call_confidence': [dict(regions=REGIONS)],
    'cn_logprob': [dict()],
    'cn_change_prob': [dict()],
}
# how the groups' answers join: the keys that are no arrays with a restart axis
JOIN = {'region_cn_extremes': dict(shared=('bins', 'first_level')), 'region_cn_moments': dict(shared=('length',)),
        'event_joint': dict(each=('p_parts',)), 'region_call': dict(extend=('cn',))}
LENGTH_EDGES = np.array([0., 1e2, 1e4, 1e6, 1e8, np.inf])
MODEL_ORDER_PATH = ('posterior_summary', 'conditional_summary')      # their model level takes a path in model segment order


def _maps(m):
    return m.seg_fwd_remap, m.seg_is_original, m.is_telomere


# the call every query should make for restarts r0 .. r0+nr-1: (batch, r0, nr, their models, their calls' states, the arguments)
DIRECT = {
    'posterior_summary': lambda b, r0, nr, ms, st, a: [dict((k, v[m.seg_fwd_remap]) for k, v in s.items()) for s, m in zip(
        posteriors.batch_summaries(b, r0, nr, states=st, marginals=a['marginals']), ms)],
    'region_events': lambda b, r0, nr, ms, st, a: posteriors.batch_region_events(b, r0, nr, a['regions'], *_maps(ms[0])),
    'region_change_counts': lambda b, r0, nr, ms, st, a: posteriors.batch_region_change_counts(b, r0, nr, a['regions'], *_maps(ms[0]), bins=a['bins']),
    'region_cn_extremes': lambda b, r0, nr, ms, st, a: posteriors.batch_region_cn_extremes(
        b, r0, nr, a['regions'], *_maps(ms[0]), quantity=a['quantity'], clone=a['clone'], bins=a['bins'], first_level=a['first_level']),
    'region_clone_extremes': lambda b, r0, nr, ms, st, a: posteriors.batch_clone_extremes(b, r0, nr, a['regions'], *_maps(ms[0]), bins=a['bins']),
    'region_cn_moments': lambda b, r0, nr, ms, st, a: posteriors.batch_region_cn_moments(b, r0, nr, a['regions'], *_maps(ms[0]), ms[0].l1),
    'event_extent': lambda b, r0, nr, ms, st, a: posteriors.batch_event_extents(b, r0, nr, a['anchors'], a['event'], a['window'], *_maps(ms[0])),
    'conditional_summary': lambda b, r0, nr, ms, st, a: posteriors.batch_conditional_summary(
        b, r0, nr, a['regions'], a['event'], a['window'], *_maps(ms[0]), marginals=a['marginals'], states=st),
    'event_span': lambda b, r0, nr, ms, st, a: posteriors.batch_event_spans(b, r0, nr, a['anchors'], a['event'], a['window'], *_maps(ms[0]), ms[0].l1),
    'event_joint': lambda b, r0, nr, ms, st, a: posteriors.batch_event_joint(b, r0, nr, a['patterns'], *_maps(ms[0])),
    'focal_events': lambda b, r0, nr, ms, st, a: posteriors.batch_focal_events(b, r0, nr, a['regions'], a['flank'], *_maps(ms[0])),
    'breakend_changes': lambda b, r0, nr, ms, st, a: posteriors.batch_breakend_changes(
        b, r0, nr, ms[0].breakpoint_idx, ms[0].num_breakpoints, ms[0].is_telomere, ms[0].seg_is_original),
    'region_call': lambda b, r0, nr, ms, st, a: posteriors.batch_region_calls(b, r0, nr, a['regions'], *_maps(ms[0]), event=a['event'], cn=st),
    'region_alternatives': lambda b, r0, nr, ms, st, a: posteriors.batch_region_alternatives(
        b, r0, nr, a['regions'], *_maps(ms[0]), k=a['k'], event=a['event'], cn=st),
    'call_confidence': lambda b, r0, nr, ms, st, a: posteriors.batch_call_confidence(b, r0, nr, st, a['regions'], *_maps(ms[0])),
    'cn_logprob': lambda b, r0, nr, ms, st, a: posteriors.batch_cn_logprob(b, r0, nr, st[:, None], ms[0].seg_is_original, ms[0].is_telomere)[:, 0],
    'cn_change_prob': lambda b, r0, nr, ms, st, a: posteriors.batch_change_prob(b, r0, nr, *_maps(ms[0])),
}


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


@pytest.fixture(scope='module')
def scenario():
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=MAX_CN, num_chains=3, seed=4)
    return e, synthetic.make_init_params(e, R, MAX_CN)


def _same(a, b, where):
    """Bit for bit, NaN equal to NaN, through dicts and lists; the same types of containers."""
    if isinstance(a, dict) or isinstance(b, dict):
        assert isinstance(a, dict) and isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], '%s[%r]' % (where, k))
    elif isinstance(a, (list, tuple)) or isinstance(b, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, '%s[%d]' % (where, i))
    elif callable(a) or callable(b):      # (length_cdf of a span summary: a function of edges, compared through its values)
        assert callable(a) and callable(b), where
        _same(a(LENGTH_EDGES), b(LENGTH_EDGES), where + '(edges)')
    else:
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (where, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'), where


def _filled(name, given):
    """The arguments with the method's defaults filled in."""
    bound = inspect.signature(getattr(restarts.RestartSet, name)).bind(None, **given)
    bound.apply_defaults()
    return dict(bound.arguments)


def _strip(name, out):
    """One restart's result without its restart axis."""
    if isinstance(out, dict):
        rule = JOIN.get(name, {})
        return dict((k, v if k in rule.get('shared', ()) else [x[0] for x in v] if k in rule.get('each', ()) else v[0]) for k, v in out.items())
    assert len(out) == 1
    return out[0]


def _by_breakpoint(arrays, model, restart_axis):
    return dict((bp, dict((k, v[:, i] if restart_axis else v[i]) for k, v in arrays.items())) for i, bp in enumerate(model.breakpoints))


def _cases(entry):
    """(the example arguments, whether cn is given) of an entry: with cn where it takes one, and with cn=None."""
    for given in EXAMPLES[entry.name]:
        for with_cn in ((True, False) if entry.cn else (False,)):
            yield given, with_cn


def test_every_query_has_examples():
    assert sorted(EXAMPLES) == sorted(DIRECT) == sorted(e.name for e in queries.QUERIES)
    for name, rule in JOIN.items():
        e = queries.BY_NAME[name]
        assert dict(shared=e.shared, extend=e.extend, each=e.each) == dict(dict(shared=(), extend=(), each=()), **rule)


def test_model_and_set_levels(hip, scenario):
    e, ps = scenario
    rs = restarts.RestartSet(e, ps, MAX_CN, num_clones=3, quiet=True, seeds=list(range(R)), options={'fb_nv': 1})
    try:
        rs.variational_update(2)
        b, models = rs.batch, rs.models
        # the regions are what the module says of them
        cs, ce = posteriors.chains_from_telomeres(models[0].is_telomere)
        chain = np.searchsorted(ce, models[0].seg_fwd_remap, side='left')
        assert len(cs) == 3 and chain[2] == chain[7] and chain[10] != chain[30] and chain[0] != chain[39]
        cns = [x['cn'] for x in rs.results()]
        # a call given in experiment order has state 0 at the model's inserted segments; the decoded path has its own states there
        given_states = np.stack([posteriors.states_in_model_order(cns[r], b, m.seg_fwd_remap) for r, m in enumerate(models)])
        model_paths = b.infer_cn_batch(0, R)[0]                                               # (R, N1, M, 2), model segment order
        decoded = posteriors.cn_to_states(model_paths, b.cn_classes, b.seg_class)
        for entry in queries.QUERIES:
            name = entry.name
            for given, with_cn in _cases(entry):
                a = _filled(name, given)
                where = '%s%r cn %s' % (name, given, with_cn)
                st = None if not entry.cn or (entry.cn == 'path' and not with_cn) else given_states if with_cn else decoded
                want = DIRECT[name](b, 0, R, models, st, a)
                if name == 'breakend_changes' and not a['arrays']:
                    want = _by_breakpoint(want, models[0], True)
                got = getattr(rs, name)(**dict(given, **({'cn': cns} if with_cn else {})))
                _same(got, want, 'set: ' + where)
                if with_cn and name in MODEL_ORDER_PATH:
                    st = decoded                               # (the model level takes the model-order path whole)
                for r, m in enumerate(models):
                    one = DIRECT[name](b, r, 1, models[r:r + 1], None if st is None else st[r:r + 1], a)
                    one = float(one[0]) if name == 'cn_logprob' else _strip(name, one)
                    if name == 'breakend_changes' and not a['arrays']:
                        one = _by_breakpoint(one, m, False)
                    cn = {} if not with_cn else {'cn': model_paths[r] if name in MODEL_ORDER_PATH else cns[r]}
                    got = getattr(m, name)(**dict(given, **cn))
                    assert name != 'cn_logprob' or type(got) is float
                    _same(got, one, 'model %d: %s' % (r, where))
        # the model level's cn_logprob of several calls at once
        several = np.stack(cns[:3])
        _same(models[1].cn_logprob(several),
              posteriors.batch_cn_logprob(b, 1, 1, np.stack([posteriors.states_in_model_order(c, b, models[1].seg_fwd_remap) for c in several])[None],
                                          models[1].seg_is_original, models[1].is_telomere)[0], 'cn_logprob of three calls')
    finally:
        rs.close()


def test_groups_level(hip, scenario):
    e, ps = scenario
    g = restarts.RestartGroups(e, ps, MAX_CN, groups=2, num_clones=3, quiet=True, seeds=list(range(R)), options={'fb_nv': 1})
    try:
        g.variational_update(2)
        g.synchronize()
        assert [len(rs.models) for rs in g.sets] == [2, 2]
        cns = [x['cn'] for x in g.results()]
        for entry in queries.QUERIES:
            name = entry.name
            for given, with_cn in _cases(entry):
                keyed = name == 'breakend_changes' and not _filled(name, given)['arrays']
                parts = [getattr(rs, name)(**dict(given, **dict({'cn': cns[sl]} if with_cn else {}, **({'arrays': True} if keyed else {}))))
                         for rs, sl in zip(g.sets, g.slices)]
                want = restarts._join(parts, **JOIN.get(name, {}))
                if keyed:
                    want = _by_breakpoint(want, g.models[0], True)
                got = getattr(g, name)(**dict(given, **({'cn': cns} if with_cn else {})))
                _same(got, want, 'groups: %s%r cn %s' % (name, given, with_cn))
                first = got if not isinstance(got, dict) else [v for k, v in got.items() if k not in JOIN.get(name, {}).get('shared', ())][0]
                assert keyed or len(first[0] if name == 'event_joint' and isinstance(first, list) else first) == R, name
    finally:
        g.close()


def test_datasets_level(hip, scenario):
    e, ps = scenario
    dg = restarts.DatasetGroups([e, e], [ps[:2], ps[2:]], MAX_CN, seeds=[[0, 1], [2, 3]], num_clones=3, quiet=True, options={'fb_nv': 1})
    try:
        dg.variational_update(2)
        dg.synchronize()
        cns = [[x['cn'] for x in part] for part in dg.results_by_dataset()]
        for entry in queries.QUERIES:
            name = entry.name
            for given, with_cn in _cases(entry):
                want = [getattr(part, name)(**dict(given, **({'cn': cns[d]} if with_cn else {}))) for d, part in enumerate(dg.parts)]
                if name == 'posterior_summary':      # (dataset after dataset in one list)
                    want = want[0] + want[1]
                got = getattr(dg, name)(**dict(given, **({'cn': cns} if with_cn else {})))
                assert len(got) == (4 if name == 'posterior_summary' else 2)
                _same(got, want, 'datasets: %s%r cn %s' % (name, given, with_cn))
    finally:
        dg.close()
