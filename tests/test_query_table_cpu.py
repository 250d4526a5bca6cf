"""The table of posterior queries (remixt_amd/queries.py) and the four class levels it gives their methods: the signatures
of the hand-written methods it replaced, what every level forwards to posteriors.batch_* and how it puts the results together
(stand-in batches, no device), and what happens without the batched kernel module."""
import inspect
import types

import numpy as np
import pytest

from remixt_amd import cn_model, posteriors, queries, restarts, synthetic
from tests import helpers as H

LEVEL_CLASSES = (cn_model.BreakpointModel, restarts.RestartSet, restarts.RestartGroups, restarts.DatasetGroups)

# str(inspect.signature(...)) of the hand-written methods, generated from the commit before the table
SIGNATURES = {
    'posterior_summary': '(self, cn=None, marginals=False)',
    'region_events': '(self, regions)',
    'region_change_counts': '(self, regions, bins=8)',
    'region_cn_extremes': "(self, regions, quantity='total', clone='any', bins=16, first_level=0)",
    'region_clone_extremes': '(self, regions, bins=16)',
    'region_cn_moments': '(self, regions)',
    'event_extent': '(self, anchors, event, window=64)',
    'conditional_summary': "(self, regions, event, window='chain', cn=None, marginals=False)",
    'event_span': '(self, anchors, event, window=64)',
    'event_joint': '(self, patterns)',
    'focal_events': '(self, regions, flank=1)',
    'breakend_changes': '(self, arrays=False)',
    'region_call': '(self, regions, event=None, cn=None)',
    'region_alternatives': '(self, regions, k=4, event=None, cn=None)',
    'call_confidence': '(self, regions, cn=None)',
    'cn_logprob': '(self, cn=None)',
    'cn_change_prob': '(self)',
}
# the same at all four levels, but for DatasetGroups.region_call, which had no `cn` ('(self, regions, event=None)') and gained it
PARENT_EXCEPTIONS = {('DatasetGroups', 'region_call'): '(self, regions, event=None)'}

# the posteriors function behind every query, and the name under which it takes the calls' states
BATCH = {
    'posterior_summary': ('batch_summaries', 'states'), 'region_events': ('batch_region_events', None),
    'region_change_counts': ('batch_region_change_counts', None), 'region_cn_extremes': ('batch_region_cn_extremes', None),
    'region_clone_extremes': ('batch_clone_extremes', None), 'region_cn_moments': ('batch_region_cn_moments', None),
    'event_extent': ('batch_event_extents', None), 'conditional_summary': ('batch_conditional_summary', 'states'),
    'event_span': ('batch_event_spans', None), 'event_joint': ('batch_event_joint', None), 'focal_events': ('batch_focal_events', None),
    'breakend_changes': ('batch_breakend_changes', None), 'region_call': ('batch_region_calls', 'cn'),
    'region_alternatives': ('batch_region_alternatives', 'cn'), 'call_confidence': ('batch_call_confidence', 'states'),
    'cn_logprob': ('batch_cn_logprob', 'states'), 'cn_change_prob': ('batch_change_prob', None),
}
DECODED_WHEN_NONE = ('region_call', 'region_alternatives', 'call_confidence', 'cn_logprob')      # cn=None: the decoded paths
SHARED = {'region_cn_extremes': ('bins', 'first_level'), 'region_cn_moments': ('length',)}

N, N1, M, K = 5, 6, 3, 2      # experiment segments, model segments, clones, breakpoints
REGIONS = [(0, 1), (2, 4), (3, 3)]
PATTERNS = [[(0, 1, 'loh'), (3, 4, 'hdel')], [(2, 2, 'loh')], [(0, 0, 'loh'), (1, 1, 'loh'), (4, 4, 'loh')]]
ARGS = {
    'posterior_summary': dict(marginals=True), 'region_events': dict(regions=REGIONS), 'region_change_counts': dict(regions=REGIONS, bins=5),
    'region_cn_extremes': dict(regions=REGIONS, quantity='major', clone=1, bins=7, first_level=2),
    'region_clone_extremes': dict(regions=REGIONS, bins=6), 'region_cn_moments': dict(regions=REGIONS),
    'event_extent': dict(anchors=[1, 3], event='loh', window=9), 'conditional_summary': dict(regions=REGIONS, event='hdel', window=3, marginals=True),
    'event_span': dict(anchors=[1, 3], event='loh', window=(2, 3)), 'event_joint': dict(patterns=PATTERNS),
    'focal_events': dict(regions=REGIONS, flank=2), 'breakend_changes': dict(arrays=True), 'region_call': dict(regions=REGIONS, event=('hdel', None)),
    'region_alternatives': dict(regions=REGIONS, k=3, event=(None, 'total')), 'call_confidence': dict(regions=REGIONS), 'cn_logprob': dict(),
    'cn_change_prob': dict(),
}


def test_the_table_names_every_query_once():
    assert [e.name for e in queries.QUERIES] == list(SIGNATURES) == list(BATCH) == list(ARGS)
    for e in queries.QUERIES:
        assert hasattr(posteriors, BATCH[e.name][0]) and e.lacks.startswith('has no ') and e.needs.endswith('_raw')
        assert (e.cn is not None) == ('cn' in inspect.signature(e.call).parameters)
    from remixt_amd import bpmodel
    assert all(hasattr(bpmodel.RemixtBatch, e.needs) for e in queries.QUERIES)


def test_the_table_loads_without_a_cycle():
    """cn_model and restarts import queries when they load: queries and what it imports of the package (posteriors) import
    neither of them, nor anything else of the package, at module level."""
    import ast

    def package_imports(module):
        with open(module.__file__) as fh:
            tree = ast.parse(fh.read())
        found = set()
        for node in tree.body:                                       # module level only: imports inside functions run later
            if isinstance(node, ast.ImportFrom) and node.level > 0:
                found.update([node.module] if node.module else [a.name for a in node.names])
            elif isinstance(node, ast.Import):
                found.update(a.name for a in node.names if a.name.startswith('remixt_amd'))
        return found
    assert package_imports(queries) == {'posteriors'} and package_imports(posteriors) == set()


def test_signatures_and_help():
    for cls in LEVEL_CLASSES:
        for name, want in SIGNATURES.items():
            method = getattr(cls, name)
            assert name in vars(cls) and inspect.isfunction(method), (cls, name)
            assert str(inspect.signature(method)) == want, (cls, name)
            if (cls.__name__, name) in PARENT_EXCEPTIONS:
                assert want == PARENT_EXCEPTIONS[(cls.__name__, name)][:-1] + ', cn=None)'
            assert method.__doc__ and method.__doc__.strip() and method.__name__ == name and method.__qualname__ == '%s.%s' % (cls.__name__, name)
        # the hand-written neighbours stay
        assert all(hasattr(cls, name) for name in ('sample_cn', 'restart_overlap') if cls is not cn_model.BreakpointModel)
    assert hasattr(cn_model.BreakpointModel, 'sample_cn') and hasattr(cn_model.BreakpointModel, 'ploidy_posterior_sd')
    # the long help of the model level survives, the restart levels say what comes back
    assert 'p_no_total_change' in cn_model.BreakpointModel.region_events.__doc__
    assert 'Suppose it is so' in cn_model.BreakpointModel.conditional_summary.__doc__
    assert '(restarts, len(regions))' in restarts.RestartSet.region_events.__doc__
    assert 'per dataset' in restarts.DatasetGroups.call_confidence.__doc__
    with pytest.raises(TypeError):
        restarts.RestartSet.region_events(None)                    # a missing argument is a TypeError, as of a plain method
    with pytest.raises(TypeError):
        restarts.RestartSet.region_events(None, REGIONS, bins=3)


# ---- stand-ins: batches that are never called, posteriors.batch_* that record and answer with the restarts' tags -------------
def _arr(tags, *shape):
    return np.stack([np.full(shape, float(t)) for t in tags])


def _nreg(a):
    return len(a['regions'])


RESULTS = {      # (tags of the restarts asked for, the arguments) -> a result of the real function's form, restart r's entries = tags[r]
    'batch_summaries': lambda t, a: [{'p_loh': np.full(N1, float(x)), 'cn_mpm': np.full((N1, M), int(x))} for x in t],
    'batch_region_events': lambda t, a: {'p_all_loh': _arr(t, _nreg(a)), 'p_no_change': _arr(t, _nreg(a))},
    'batch_region_change_counts': lambda t, a: {'num_changes': _arr(t, _nreg(a), a['bins'])},
    'batch_region_cn_extremes': lambda t, a: {'bins': a['bins'], 'first_level': a['first_level'], 'peak_pmf': _arr(t, _nreg(a), a['bins']),
                                              'peak_q50': _arr(t, _nreg(a)).astype(np.int64)},
    'batch_clone_extremes': lambda t, a: {'peak_total_pmf': _arr(t, _nreg(a), M - 1, a['bins'])},
    'batch_region_cn_moments': lambda t, a: {'length': np.arange(_nreg(a)) + 1., 'total_cn_mean': _arr(t, _nreg(a), M), 'total_cn_cov': _arr(t, _nreg(a), M, M)},
    'batch_event_extents': lambda t, a: [[{'p_event': float(x), 'anchor': an} for an in a['anchors']] for x in t],
    'batch_conditional_summary': lambda t, a: [[{'log_evidence': float(x), 'region': rg} for rg in a['regions']] for x in t],
    'batch_event_spans': lambda t, a: [[{'p_event': float(x), 'anchor': an} for an in a['anchors']] for x in t],
    'batch_event_joint': lambda t, a: {'p_joint': _arr(t, len(a['patterns'])), 'p_parts': [_arr(t, len(p)) for p in a['patterns']]},
    'batch_focal_events': lambda t, a: {'p_focal_loh': _arr(t, _nreg(a))},
    'batch_breakend_changes': lambda t, a: {'p_change': _arr(t, K, 2), 'p_change_both': _arr(t, K)},
    'batch_region_calls': lambda t, a: {'cn': [[np.full((2, M, 2), int(x)) for _ in a['regions']] for x in t], 'log_prob': _arr(t, _nreg(a))},
    'batch_region_alternatives': lambda t, a: [[{'log_prob': np.full(a['k'], float(x))} for _ in a['regions']] for x in t],
    'batch_call_confidence': lambda t, a: {'p_call': _arr(t, _nreg(a))},
    'batch_cn_logprob': lambda t, a: np.stack([np.full(np.shape(a['states'])[1], float(x)) for x in t]),
    'batch_change_prob': lambda t, a: _arr(t, N - 1),
}


class _Batch(object):
    """A batch whose restart r carries the tag first + r; it has every *_raw method's name and decodes to paths of 100 + tag."""
    num_segments = N1
    cn_classes = 'classes'
    seg_class = 'seg_class'

    def __init__(self, first, count):
        self.first, self.count = first, count
        for e in queries.QUERIES:
            setattr(self, e.needs, None)

    def infer_cn_batch(self, r0, nr):
        assert (r0, nr) == (0, self.count)
        return np.stack([np.full((N1, M, 2), 100 + self.first + r) for r in range(nr)]), None


def _model(batch, r, maps):
    m = object.__new__(cn_model.BreakpointModel)

    def infer_cn(path):
        path[:] = 100 + batch.first + r
    m.model = types.SimpleNamespace(_batch=batch, _r=r, num_segments=N1, num_clones=M, num_alleles=2, infer_cn=infer_cn)
    m.__dict__.update(maps)
    return m


def _maps():
    """One dataset's segment maps and breakpoints: objects of its own, so that a level that took another dataset's shows."""
    return dict(seg_fwd_remap=np.array([0, 1, 3, 4, 5]), seg_is_original=np.array([1, 1, 0, 1, 1, 1], dtype=bool), is_telomere=np.zeros(N1, dtype=bool),
                l1=np.arange(N1) + 1., breakpoint_idx=np.array([0, -1, 1, 0, 1, -1]), num_breakpoints=K, breakpoints=['bp_a', 'bp_b'])


def _set(first, count, maps):
    rs = object.__new__(restarts.RestartSet)
    rs.batch = _Batch(first, count)
    rs.models = [_model(rs.batch, r, maps) for r in range(count)]
    return rs


def _groups(first):
    """3 restarts in groups of 2 + 1, tags first .. first + 2."""
    g = object.__new__(restarts.RestartGroups)
    maps = _maps()
    g.sets = [_set(first, 2, maps), _set(first + 2, 1, maps)]
    g.slices = [slice(0, 2), slice(2, 3)]
    g.models = [m for rs in g.sets for m in rs.models]
    g._pool = None
    return g


def _datasets():
    d = object.__new__(restarts.DatasetGroups)
    d.parts = [_groups(0), _groups(10)]
    d._pool, d._workers = None, 2
    return d


@pytest.fixture
def calls(monkeypatch):
    """Every posteriors.batch_* of the table replaced by a recorder with the real function's signature: (name, arguments) per call."""
    log = []

    def fake(name):
        signature = inspect.signature(getattr(posteriors, name))

        def recorder(*args, **kwargs):
            bound = signature.bind(*args, **kwargs)
            bound.apply_defaults()
            a = dict(bound.arguments)
            log.append((name, a))
            return RESULTS[name]([a['batch'].first + a['r0'] + i for i in range(a['nr'])], a)
        return recorder
    for name, _ in BATCH.values():
        monkeypatch.setattr(posteriors, name, fake(name))
    # a path's states: its own first entry at every segment (all paths here are constant)
    monkeypatch.setattr(posteriors, 'cn_to_states', lambda cn, cn_classes, seg_class: np.asarray(cn)[..., 0, 0].astype(np.int16))
    monkeypatch.setattr(posteriors, 'states_in_model_order', lambda cn, batch, remap: np.full(batch.num_segments, np.asarray(cn).flat[0], dtype=np.int16))
    return log


def _same(a, b, where=''):
    assert type(a) is type(b), (where, type(a), type(b))
    if isinstance(a, dict):
        assert list(a) == list(b), (where, list(a), list(b))
        for k in a:
            _same(a[k], b[k], '%s[%r]' % (where, k))
    elif isinstance(a, list):
        assert len(a) == len(b), (where, len(a), len(b))
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, '%s[%d]' % (where, i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (where, a, b)
    else:
        assert a == b, (where, a, b)


def _want(name, tags, maps, **user):
    """What a restart level returns for restarts of these tags: the posteriors function's answer for all of them at once."""
    a = inspect.signature(getattr(restarts.RestartSet, name)).bind(None, **user)
    a.apply_defaults()
    a = dict(a.arguments, states=np.zeros((len(tags), 1, N1)))
    out = RESULTS[BATCH[name][0]](tags, a)
    if name == 'posterior_summary':
        return [dict((k, v[maps['seg_fwd_remap']]) for k, v in s.items()) for s in out]
    if name == 'cn_logprob':
        return out[:, 0]
    return out


def _strip(name, out):
    """The restart axis of a result of one restart taken off."""
    if name == 'cn_logprob':
        assert out.shape == (1,)
        return float(out[0])
    if isinstance(out, dict):
        return dict((k, v if k in SHARED.get(name, ()) else [p[0] for p in v] if k == 'p_parts' else v[0]) for k, v in out.items())
    assert len(out) == 1
    return out[0]


def _check_call(rec, name, batch, r0, nr, model, user, cn_tags):
    """One recorded call: the function, the restarts, the user's arguments, the model's maps, and the calls' states row by row."""
    fn, a = rec
    bname, cn_key = BATCH[name]
    assert fn == bname and a['batch'] is batch and (a['r0'], a['nr']) == (r0, nr), (name, fn, a['r0'], a['nr'])
    for k, v in user.items():
        if k not in ('cn', 'arrays'):
            assert a[k] is v or a[k] == v, (name, k)          # (every other argument of the user's reaches the function under its name)
    for k in ('seg_fwd_remap', 'seg_is_original', 'is_telomere', 'l1', 'breakpoint_idx', 'num_breakpoints'):
        if k in a:
            assert a[k] is getattr(model, k), (name, k)
    if cn_key is not None:
        if cn_tags is None:
            assert a[cn_key] is None, name
        else:
            states = np.asarray(a[cn_key])
            assert states.dtype == np.int16 and states.shape[0] == nr and states.shape[-1] == N1, (name, states.shape)
            assert np.array_equal(states.reshape(nr, -1), np.repeat(np.array(cn_tags)[:, None], states[0].size, axis=1)), (name, states, cn_tags)


def _cn_cases(name, tags):
    """(cn per restart or None, the states each restart's call must show) for a query: its paths given, and cn=None."""
    if BATCH[name][1] is None:
        return [(None, None)]
    return [([np.full((N, M, 2), t) for t in tags], list(tags)), (None, [100 + t for t in tags] if name in DECODED_WHEN_NONE else None)]


@pytest.mark.parametrize('name', list(SIGNATURES))
def test_model_and_set_forward_and_assemble(name, calls):
    maps = _maps()
    rs = _set(0, 3, maps)
    for cn, cn_tags in _cn_cases(name, [0, 1, 2]):
        user = dict(ARGS[name], **({} if BATCH[name][1] is None else {'cn': cn}))
        del calls[:]
        got = getattr(rs, name)(**user)
        assert len(calls) == 1
        _check_call(calls[0], name, rs.batch, 0, 3, rs.models[0], user, cn_tags)
        _same(got, _want(name, [0, 1, 2], maps, **ARGS[name]), name)
        # the model level: its restart alone, exactly the restart axis gone
        for r, m in enumerate(rs.models):
            one = dict(ARGS[name])
            if BATCH[name][1] is not None:
                # (posterior_summary and conditional_summary take the model level's path in model segment order)
                one['cn'] = None if cn is None else np.full((N1, M, 2), r) if name in ('posterior_summary', 'conditional_summary') else cn[r]
            del calls[:]
            got = getattr(m, name)(**one)
            assert len(calls) == 1
            _check_call(calls[0], name, rs.batch, r, 1, m, one, None if cn_tags is None else cn_tags[r:r + 1])
            _same(got, _strip(name, _want(name, [r], maps, **ARGS[name])), '%s of model %d' % (name, r))


@pytest.mark.parametrize('name', list(SIGNATURES))
def test_groups_and_datasets_forward_and_assemble(name, calls):
    g = _groups(0)
    for cn, cn_tags in _cn_cases(name, [0, 1, 2]):
        user = dict(ARGS[name], **({} if BATCH[name][1] is None else {'cn': cn}))
        del calls[:]
        got = getattr(g, name)(**user)
        assert len(calls) == 2
        for rs, sl in zip(g.sets, g.slices):      # (the groups run on threads: the calls come in any order)
            rec = [c for c in calls if c[1]['batch'] is rs.batch]
            assert len(rec) == 1
            _check_call(rec[0], name, rs.batch, 0, len(rs.models), rs.models[0], user, None if cn_tags is None else cn_tags[sl])
        want = _want(name, [0, 1, 2], g.models[0].__dict__, **ARGS[name])
        _same(got, want, name)
        if isinstance(want, dict):      # shared keys come once, the others along all restarts
            for k, v in got.items():
                assert (v is not None and k in SHARED.get(name, ())) or len(v[0] if k == 'p_parts' else v) == 3, (name, k)
    d = _datasets()
    tags = [[0, 1, 2], [10, 11, 12]]
    for case in range(2):
        per = [_cn_cases(name, t)[min(case, len(_cn_cases(name, t)) - 1)] for t in tags]
        user = dict(ARGS[name], **({} if BATCH[name][1] is None else {'cn': None if per[0][0] is None else [p[0] for p in per]}))
        del calls[:]
        got = getattr(d, name)(**user)
        assert len(calls) == 4
        for part, (_, cn_tags) in zip(d.parts, per):
            for rs, sl in zip(part.sets, part.slices):
                rec = [c for c in calls if c[1]['batch'] is rs.batch]
                assert len(rec) == 1
                _check_call(rec[0], name, rs.batch, 0, len(rs.models), rs.models[0], user, None if cn_tags is None else cn_tags[sl])
        want = [_want(name, t, part.models[0].__dict__, **ARGS[name]) for t, part in zip(tags, d.parts)]
        if name == 'posterior_summary':      # (its datasets come strung together, dataset after dataset)
            want = want[0] + want[1]
        _same(got, want, name)


def test_breakend_changes_by_breakpoint_at_every_level(calls):
    d = _datasets()
    g = d.parts[1]
    rs, m = g.sets[0], g.sets[0].models[1]
    arrays = RESULTS['batch_breakend_changes']([10, 11, 12], {})
    got = g.breakend_changes()
    assert list(got) == ['bp_a', 'bp_b']
    for i, bp in enumerate(got):
        _same(got[bp], dict((k, v[:, i]) for k, v in arrays.items()), bp)
    _same(rs.breakend_changes(arrays=False), dict((bp, dict((k, v[:2]) for k, v in x.items())) for bp, x in got.items()))
    _same(m.breakend_changes(), dict((bp, dict((k, v[1]) for k, v in x.items())) for bp, x in got.items()))
    both = d.breakend_changes()
    assert len(both) == 2 and list(both[0]) == ['bp_a', 'bp_b']
    _same(both[1], got)
    _same(d.breakend_changes(True)[1], arrays)


def test_model_level_calls(calls):
    rs = _set(0, 2, _maps())
    m = rs.models[1]
    several = np.stack([np.full((N, M, 2), t) for t in (4, 5, 6)])
    got = m.cn_logprob(several)
    assert isinstance(got, np.ndarray) and got.shape == (3,) and (got == 1.).all()
    states = calls[-1][1]['states']
    assert states.shape == (1, 3, N1) and np.array_equal(states[0, :, 0], [4, 5, 6]) and (calls[-1][1]['r0'], calls[-1][1]['nr']) == (1, 1)
    assert type(m.cn_logprob(several[0])) is float and type(m.cn_logprob()) is float
    for name in ('region_call', 'region_alternatives', 'call_confidence'):
        with pytest.raises(ValueError, match=r'%s takes one call of shape \(num_segments, num_clones, 2\)' % name):
            getattr(m, name)(REGIONS, cn=several)


# ---- without the batched kernel module ---------------------------------------------------------------------------------------
def test_without_the_kernel():
    from oracle import oracle
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    e = synthetic.make_experiment(30, num_clones=3, max_copy_number=3, num_chains=2, seed=1)
    rs = restarts.RestartSet(e, synthetic.make_init_params(e, 2, 3), 3, num_clones=3, quiet=True, kernel_module=oracle, seeds=[0, 1])
    assert rs.batch is None
    args = dict(ARGS, event_extent=dict(anchors=[1], event='loh'), event_span=dict(anchors=[1], event='loh'))
    for entry in queries.QUERIES:
        with pytest.raises(NotImplementedError, match='kernel module .*oracle.* %s$' % entry.lacks):
            getattr(mo, entry.name)(**args[entry.name])
        with pytest.raises(NotImplementedError, match=entry.lacks):
            getattr(rs, entry.name)(**args[entry.name])
    cn = [np.zeros((30, 3, 2), dtype=int)] * 2
    with pytest.raises(NotImplementedError, match='posterior summaries against a decoded path need the batched kernel module'):
        rs.posterior_summary(cn=cn)
    with pytest.raises(NotImplementedError, match='conditional summaries against a decoded path need the batched kernel module'):
        rs.conditional_summary([(0, 1)], 'hdel', cn=cn)
    with pytest.raises(NotImplementedError, match='has no region decode'):
        rs.region_call([(0, 1)], cn=cn)
