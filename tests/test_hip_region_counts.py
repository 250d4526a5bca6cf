"""Region change counts on the device (rmx_region_counts / k_region_counts): against the log-domain numpy twin on the
read-back framelogprob / log_transmat, the identities that tie the bins to rmx_region_prob, the sampler, two state
classes, the mixed transition model, inserted segments, invariance to batching and grouping, no side effects on the
model, errors, the pipeline, and a long run."""
import time

import numpy as np
import pytest

from remixt_amd import posteriors, synthetic
from tests import helpers as H
from tests import region_counts_twin
from tests.test_hip_region_events import LABELS, MASKS, Case
from tests.test_hip_sample_cn import GRIDS, _fitted, _model_state, _pipeline_case, _same_results

pytestmark = pytest.mark.gpu

U = 2. ** -53
BINS = (1, 5, 16)
# (mask, label) of every constraint a query is run with: each label alone, two of mask + label
CONSTRAINTS = [(None, k) for k in LABELS] + [('not_loh', 'total'), ('not_subclonal', 'unphased')]


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


class CountsCase(Case):
    def __init__(self, *args, **kw):
        Case.__init__(self, *args, **kw)
        self.ctwin = region_counts_twin.CountsTwin.sharing(self.twin)

    def counts(self, runs, K, constraints=CONSTRAINTS, r0=None, nr=1):
        q = np.array([[a, b, -1 if mk is None else MASKS.index(mk), LABELS.index(lb)] for (a, b) in runs for (mk, lb) in constraints], dtype=np.int32)
        out = self.b.region_counts_raw(self.r if r0 is None else r0, nr, q, self.masks, self.labels, self.constrain, K)
        return out.reshape(nr, len(runs), len(constraints), K)

    def want_counts(self, a, b, K, mk, lb):
        return self.ctwin.logcounts(a, b, K, self.label_seg[lb], None if mk is None else self.mask_seg[mk], self.constrain)

    def check_counts(self, runs, bins=BINS, constraints=CONSTRAINTS, tag=''):
        worst = 0.
        for K in bins:
            got = self.counts(runs, K, constraints)[0]
            for i, (a, b) in enumerate(runs):
                L = b - a + 1
                for j, (mk, lb) in enumerate(constraints):
                    want = self.want_counts(a, b, K, mk, lb)
                    err = np.abs(np.exp(got[i, j]) - np.exp(want))
                    worst = max(worst, err.max() / L)
                    print('%s K %d run [%d, %d] mask %s label %s: max |P - twin| %.3e, P %s' % (tag, K, a, b, mk, lb, err.max(), np.exp(got[i, j])))
                    assert (err <= L * 1e-9).all(), (tag, K, a, b, mk, lb, got[i, j], want)
                    assert np.array_equal(got[i, j] == -np.inf, want == -np.inf), (tag, K, a, b, mk, lb, got[i, j], want)
                    assert (got[i, j, L:] == -np.inf).all()      # more changes than the run has adjacencies
        print('%s worst |P - twin| / L: %.3e' % (tag, worst))


@pytest.fixture(scope='module')
def cases(hip):
    return dict(((N, M, c), CountsCase(_fitted(hip, N, M, c))) for N, M, c in GRIDS)


def _lse(lp):
    m = lp.max(axis=-1)
    with np.errstate(invalid='ignore'):
        return np.where(np.isfinite(m), m + np.log(np.exp(lp - np.where(np.isfinite(m), m, 0.)[..., None]).sum(axis=-1)), m)


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_twin(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    assert case.S == {8: 165, 12: 355, 6: 457}[max_cn] and case.S % 64
    assert case.m.num_breakpoints > 0 and (case.bidx >= 0).any()
    b = case.b
    b.profile_reset(); b.profile_enable(1)
    case.counts(case.queries(), 16)
    prof = b.profile(); b.profile_enable(0)
    assert prof['k_region_counts'][1] == 1 and prof['k_region_counts'][0] > 0
    case.check_counts(case.queries(), tag='S %d' % case.S)
    # the model-level form
    q = np.array([[a, b_, 0, 1] for a, b_ in case.queries()], dtype=np.int32)
    one = case.m.model.region_counts(q, case.masks, case.labels, case.constrain, 5)
    assert one.shape == (len(q), 5) and np.array_equal(one, b.region_counts_raw(case.r, 1, q, case.masks, case.labels, case.constrain, 5)[0])


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_identities(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    b, S, K = case.b, case.S, 16
    c = int(np.argmax(case.ce - case.cs))
    seg = np.arange(case.cs[c], case.ce[c] + 1)
    runs = [(int(a), int(e)) for a in seg for e in seg if a <= e]
    L = np.array([e - a + 1 for a, e in runs])
    # (i) without a mask the bins of a run add up to 1
    got = case.counts(runs, K, [(None, 'state'), (None, 'total')])[0]
    tot = _lse(got)
    bound = L * (4 * S + 32) * U + 16 * U
    print('S %d: max |logsumexp of the bins| %.3e over %d runs (bound of one segment %.3e)' % (S, np.abs(tot).max(), len(runs), bound.min()))
    assert (np.abs(tot) <= bound[:, None]).all()
    # (ii) bin 0 is rmx_region_prob's event with the same (mask, label)
    cons = [(None, 'state'), ('not_loh', 'total'), ('not_subclonal', 'unphased')]
    gc = case.counts(runs, K, cons)[0]
    gp = case.raw(runs, cons)[0]
    err = np.abs(np.exp(gc[..., 0]) - np.exp(gp))
    print('S %d: bin 0 against k_region_prob: max |dP| %.3e' % (S, err.max()))
    assert (err <= L[:, None] * 1e-9).all()
    # (iii) one bin is the mask-only event
    g1 = case.counts(runs, 1, cons)[0][..., 0]
    gm = case.raw(runs, [(mk, None) for mk, _ in cons])[0]
    err = np.abs(np.exp(g1) - np.exp(gm))
    print('S %d: K = 1 against the mask-only query: max |dP| %.3e' % (S, err.max()))
    assert (err <= L[:, None] * 1e-9).all()
    # (iv) where the last bin cannot saturate, the mean count is the sum of the adjacent pairs' change probabilities
    pairs = [(int(a), int(a) + 1) for a in seg[:-1]]
    if pairs:
        change = -np.expm1(np.minimum(case.raw(pairs, [(None, 'state')])[0, :, 0], 0.))
        P = np.exp(got[:, 0])
        for i, (a, e) in enumerate(runs):
            if e - a <= K - 1:
                mean = (np.arange(K) * P[i]).sum()
                want = change[a - seg[0]:e - seg[0]].sum()
                assert abs(mean - want) <= (K * (K - 1) / 2 + L[i]) * 1e-9, (a, e, mean, want)


def test_against_the_sampler(hip):
    """The masked case of test_hip_region_events.test_against_the_sampler (experiment seed 0).  The twin over the oracle
    kernel module's arrays of this case gives, among these runs and constraints with 8 bins, five (run, bin) pairs with
    0.01 < P < 0.99, all of them under ('not_subclonal', 'unphased'): with the read counts masked the transition penalty
    keeps label changes themselves below 1e-3 away from breakends, for every experiment seed 0 .. 8, so the pairs that
    test the histogram are informative through their mask."""
    from tests.test_hip_posterior_summary import _fitted as fitted_masked
    m = fitted_masked(hip, 30, 3, 8, sweeps=3, masked=True)
    case = CountsCase(m)
    NS, K = 4096, 8
    st = case.b.sample_states(case.r, 1, NS, [99]).astype(np.int64)[0]
    runs = case.queries()
    got = np.exp(case.counts(runs, K)[0])
    informative = 0
    for i, (a, e) in enumerate(runs):
        seg = np.arange(a, e + 1)
        for j, (mk, lb) in enumerate(CONSTRAINTS):
            hit = np.ones(NS, dtype=bool)
            if mk is not None:
                for n in seg[case.constrain[seg]]:
                    hit &= case.mask_seg[mk][n, st[:, n]]
            changes = np.zeros(NS, dtype=np.int64)
            for n in seg[:-1]:
                changes += case.label_seg[lb][n, st[:, n]] != case.label_seg[lb][n + 1, st[:, n + 1]]
            for k in range(K):
                P = got[i, j, k]
                freq = (hit & (np.minimum(changes, K - 1) == k)).mean()
                tol = 6 * np.sqrt(P * (1 - min(P, 1.)) / NS) + 2. / NS
                informative += 0.01 < P < 0.99
                assert abs(freq - P) <= tol, (a, e, mk, lb, k, freq, P)
    print('informative (run, constraint, bin) triples: %d' % informative)
    assert informative >= 3


def test_two_classes(hip):
    m, h, e = H.make_model(hip, N=40, M=3, max_cn=4, chains=3)
    M = 3
    classes, _ = m._state_tables(M)
    classes = np.repeat(classes[:1], 2, axis=0)
    classes[1, :, 0, :] = (1, 0)
    N = m.N1
    seg_class = (np.arange(N) % 2).astype(np.int32)                      # 0, 1, 0, 1, ...
    brk_states = m.create_brk_states(M, m.max_copy_number, m.max_copy_number_diff)
    b = hip.RemixtBatch(M, N, m.num_breakpoints, m.normal_contamination, classes, seg_class, brk_states, np.asarray(h, dtype=float)[None],
                        m.l1, m.x1[:, 2].copy(), m.x1[:, 0:2].copy(), m.is_telomere, m.breakpoint_idx, m.breakpoint_orient,
                        m.transition_log_prob, [m.divergence_weight])
    try:
        # (as test_hip_region_events.test_two_classes: the sweeps run on the total read counts alone)
        b.set_array(0, 'allele_likelihood_mask', np.zeros(N, dtype=np.int64))
        b.variational_update(2)
        case = CountsCase(m, batch=b, r=0)
        loh = case.masks[:, MASKS.index('loh')]
        assert not loh[0].any() and loh[1].any()                         # the mask differs per class
        assert np.array_equal(case.labels[0], case.labels[1])            # the labels do not
        case.check_counts(case.queries(), bins=(5,), constraints=CONSTRAINTS + [('loh', 'state')], tag='two classes')
        # (a kernel that took class 0's masks everywhere would call LOH impossible)
        odd = case.counts([(n, n) for n in range(1, N, 2)], 3, [('loh', 'state')])[0, :, 0, 0]
        even = case.counts([(n, n) for n in range(0, N, 2)], 3, [('loh', 'state')])[0, :, 0, 0]
        assert (odd[case.constrain[1::2]] > -np.inf).any() and (even[case.constrain[0::2]] == -np.inf).all()
    finally:
        b.close()


def test_mixed_transition_model(hip):
    """The snapshot of the last update_p_cn under another transition_model than the current one, both directions."""
    m = _fitted(hip, 40, 3, 4, seed=3)
    T0 = np.array(m.model.log_transmat)
    m.model.transition_model = 1
    assert np.array_equal(np.array(m.model.log_transmat), T0)            # the snapshot stays the model-0 one
    case = CountsCase(m)
    case.check_counts(case.queries(), bins=(5,), tag='mixed model')
    m2 = _fitted(hip, 40, 3, 4, seed=3, transition_model=1)
    assert m2.model.transition_model == 1
    m2.model.transition_model = 0
    case2 = CountsCase(m2)
    assert not np.array_equal(np.array(m2.model.log_transmat), T0)
    case2.check_counts(case2.queries(), bins=(16,), tag='mixed model 1 -> 0')


def test_inserted_segments(hip):
    """Two breakends on one boundary: the model inserts a zero-length segment there, and the count runs over the two
    adjacencies through it (a path that takes a third state in it changes twice)."""
    e = synthetic.make_experiment(60, num_clones=3, max_copy_number=4, num_chains=3, seed=7)
    e.breakpoints = H.add_shared_boundary_breakpoints(e)
    m, h, _ = H.make_model(hip, M=3, max_cn=4, experiment=e)
    H.attach(m, h)
    m.variational_update(); m.variational_update()
    case = CountsCase(m)
    assert m.N1 > m.N and not case.constrain.all()
    dummy = int(np.flatnonzero(~case.constrain & (np.arange(m.N1) > 0) & (case.tel == 0))[0])
    assert case.constrain[dummy - 1] and case.constrain[dummy + 1]
    case.check_counts([(dummy - 1, dummy + 1), (dummy, dummy), (dummy, dummy + 1)], bins=(1, 4), tag='inserted segment')
    # the experiment pair around it, through region_change_counts: the run holds the inserted segment, so two changes can happen
    i = int(m.seg_rev_remap[dummy - 1])
    assert m.seg_fwd_remap[i] == dummy - 1 and m.seg_fwd_remap[i + 1] == dummy + 1
    out = m.region_change_counts([(i, i + 1), (i, i)], bins=4)
    assert sorted(out) == ['num_changes', 'num_total_changes']
    for name, lb in posteriors.COUNT_LABELS:
        assert out[name].shape == (2, 4)
        assert np.abs(out[name][0] - np.exp(case.want_counts(dummy - 1, dummy + 1, 4, None, lb))).max() <= 3e-9, name
        assert np.abs(out[name][1] - [1, 0, 0, 0]).max() <= 3e-9 and out[name][0, 3] == 0, name
    assert abs(out['num_changes'][0, 0] - m.region_events([(i, i + 1)])['p_no_change'][0]) <= 3e-9


def test_invariance(hip):
    from remixt_amd.restarts import RestartGroups, RestartSet
    e = synthetic.make_experiment(80, num_clones=3, max_copy_number=4, num_chains=3, seed=4)
    ps = synthetic.make_init_params(e, 4, 4)
    rs = RestartSet(e, ps, 4, num_clones=3, quiet=True, seeds=list(range(4)))
    rs.variational_update(2)
    b, m = rs.batch, rs.models[0]
    masks, labels = posteriors.event_tables(b.cn_classes)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    regions = [(i, j) for i in range(0, 70, 7) for j in (i, i + 1, i + 9)]
    runs, _, constrain = posteriors.region_queries(regions, m.seg_fwd_remap, m.seg_is_original, cs, ce)
    q = np.array([[a, e_, mi, li] for a, e_ in runs for mi, li in ((-1, 0), (1, 1), (5, 2))], dtype=np.int32)
    K = 6
    call = lambda r0, nr, qq: b.region_counts_raw(r0, nr, qq, masks, labels, constrain, K)
    full = call(0, 4, q)
    assert full.shape == (4, len(q), K) and not np.array_equal(full[0], full[1])
    for r in range(4):
        assert np.array_equal(call(r, 1, q)[0], full[r], equal_nan=True)
    assert np.array_equal(call(1, 2, q), full[1:3], equal_nan=True)
    for i in range(0, len(q), 5):
        assert np.array_equal(call(0, 4, q[i:i + 1])[:, 0], full[:, i], equal_nan=True)
    assert np.array_equal(call(0, 4, q[::-1].copy()), full[:, ::-1], equal_nan=True)
    per_set = rs.region_change_counts(regions, bins=K)
    one = rs.models[2].region_change_counts(regions, bins=K)
    for k in posteriors.COUNT_ARRAYS:
        assert per_set[k].shape == (4, len(regions), K) and np.array_equal(per_set[k][2], one[k]), k
        assert ((per_set[k] >= 0) & (per_set[k] <= 1)).all() and np.abs(per_set[k].sum(axis=-1) - 1).max() <= 1e-9, k
    rs.close()
    groups = RestartGroups(e, ps, 4, groups=2, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    single = RestartGroups(e, ps, 4, groups=1, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    for g in (groups, single):
        g.variational_update(2)
    a, c = groups.region_change_counts(regions, bins=K), single.region_change_counts(regions, bins=K)
    for k in posteriors.COUNT_ARRAYS:
        assert a[k].shape == (4, len(regions), K) and np.array_equal(a[k], c[k]), k
    groups.close(); single.close()


def test_no_side_effects(hip):
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    before = _model_state(m1)
    out = m1.region_change_counts([(0, 10), (5, 5), (20, 49)], bins=16)
    assert set(out) == set(posteriors.COUNT_ARRAYS) and out['num_changes'].shape == (3, 16)
    after = _model_state(m1)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    # a fit continued after the call equals one without it
    for m in (m1, m2):
        m.variational_update()
    s1, s2 = _model_state(m1), _model_state(m2)
    for k in s1:
        assert np.array_equal(s1[k], s2[k], equal_nan=True), k
    assert m1.model.calculate_elbo() == m2.model.calculate_elbo()


def test_errors(hip):
    from remixt_amd import bpmodel
    m, h, e = H.make_model(hip, N=30, M=3, max_cn=3)
    H.attach(m, h)
    b, r = m.model._batch, m.model._r
    masks, labels = posteriors.event_tables(b.cn_classes)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    ok = [[int(cs[0]), int(cs[0]) + 1, 0, 0]]
    with pytest.raises(ValueError, match='update_p_cn'):
        b.region_counts_raw(r, 1, ok, masks, labels, None, 4)
    assert bpmodel.last_error_restarts() == [r]
    with pytest.raises(ValueError, match='update_p_cn'):
        m.region_change_counts([(0, 3)])
    m.variational_update()
    N = b.num_segments
    b.profile_reset(); b.profile_enable(1)
    assert b.region_counts_raw(r, 1, ok, masks, labels, None, 4).shape == (1, 1, 4)
    launches = b.profile()['k_region_counts'][1]
    assert launches == 1
    bad = [(ok, 0, 'bins'), (ok, 17, 'bins'), (ok + [[0, 1, -1, -1]], 4, 'label index'), (ok + [[3, 2, -1, 0]], 4, 'first <= last'),
           (ok + [[int(ce[0]), int(ce[0]) + 1, -1, 0]], 4, 'chain end'), (ok + [[int(cs[0]), int(ce[1]), -1, 0]], 4, 'chain end'),
           (ok + [[0, N, -1, 0]], 4, 'first <= last'), (ok + [[0, 1, len(MASKS), 0]], 4, 'mask index'), (ok + [[0, 1, -1, len(LABELS)]], 4, 'label index')]
    for q, K, text in bad:
        with pytest.raises(ValueError, match='^bad argument: .*' + text):
            b.region_counts_raw(r, 1, q, masks, labels, None, K)
        assert bpmodel.last_error_restarts() == []
        assert b.profile()['k_region_counts'][1] == launches, (q, K)      # nothing was launched
    b.profile_enable(0)
    with pytest.raises(ValueError, match='bins'):
        m.region_change_counts([(0, 3)], bins=17)
    from oracle import oracle
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError):
        mo.region_change_counts([(0, 3)])


def test_pipeline_change_counts(hip, tmp_path):
    from remixt_amd import workflow
    from remixt_amd.analysis import pipeline
    import pickle
    e, config, init_params = _pipeline_case()
    ids = sorted(init_params)
    seeds = [100 + i for i in ids]
    cn_regions = [('geneA', 10, 14), ('arm', 0, 250), ('seg', 77, 77), ('pair', 300, 301)]
    K = 6
    # (two groups of two restarts, the grouping fit_restarts_distributed and the workflow use: equal arrays throughout)
    base = pipeline.fit_restarts(e, init_params, dict(config, cn_regions=cn_regions), seeds=seeds, groups=2)
    on = pipeline.fit_restarts(e, init_params, dict(config, cn_regions=cn_regions, cn_region_change_bins=K), seeds=seeds, groups=2)
    # bins = 0 (the default): nothing of it in the results; set: the same results plus region_change_counts
    assert not any('region_change_counts' in res for res in base.values())
    for i in base:      # (_same_results compares arrays: the region events, a dict, are compared here)
        for k in posteriors.REGION_ARRAYS:
            assert np.array_equal(base[i]['region_events'][k], on[i]['region_events'][k]), (i, k)
    strip = lambda results: dict((i, dict((k, v) for k, v in res.items() if k not in ('region_events', 'region_change_counts'))) for i, res in results.items())
    _same_results(strip(base), strip(on))
    for i in ids:
        cc = on[i]['region_change_counts']
        assert cc['names'] == ['geneA', 'arm', 'seg', 'pair'] and cc['bins'] == K and sorted(cc) == ['bins', 'names', 'num_changes', 'num_total_changes']
        for k in posteriors.COUNT_ARRAYS:
            assert cc[k].shape == (4, K) and ((cc[k] >= 0) & (cc[k] <= 1)).all(), (i, k)
            assert np.abs(cc[k].sum(axis=1) - 1).max() <= 1e-9, (i, k)
        assert np.abs(cc['num_changes'][:, 0] - on[i]['region_events']['p_no_change']).max() <= 3e-9
        assert np.abs(cc['num_total_changes'][:, 0] - on[i]['region_events']['p_no_total_change']).max() <= 3e-9
        assert np.abs(cc['num_changes'][2] - np.eye(K)[0]).max() <= 1e-12      # one segment: no adjacency
    one = pipeline.fit(e, init_params[ids[1]], dict(config, cn_regions=cn_regions, cn_region_change_bins=K), quiet=True, init_id=ids[1])
    assert one['region_change_counts']['num_changes'].shape == (4, K) and one['region_change_counts']['names'] == cc['names']
    # the distributed form: the arrays through the record
    from remixt_amd import restarts
    dist = restarts.fit_restarts_distributed(e, [init_params[i] for i in ids], 4, num_clones=3, num_em_iter=config['num_em_iter'],
                                             num_update_iter=config['num_update_iter'], seeds=seeds, quiet=True, cn_regions=cn_regions,
                                             cn_region_change_bins=K, **pipeline._model_kwargs(e, config))
    for j, i in enumerate(ids):
        assert dist[j]['region_change_counts']['names'] == cc['names'] and dist[j]['region_change_counts']['bins'] == K
        for k in posteriors.COUNT_ARRAYS:
            assert np.array_equal(dist[j]['region_change_counts'][k], on[i]['region_change_counts'][k]), (i, k)
    # the workflow (fit_restarts_distributed + collate): the arrays in the record and in the store equal fit_restarts'
    exp_file = str(tmp_path / 'experiment.pickle')
    with open(exp_file, 'wb') as f:
        pickle.dump(e, f)
    workflow.fit_model(exp_file, str(tmp_path / 'r.store'), dict(config, cn_regions=cn_regions, cn_region_change_bins=K), None, seeds=seeds)
    with pipeline._Store(str(tmp_path / 'r.store'), 'r') as st:
        for i in sorted(st['stats']['init_id']):
            for k in posteriors.COUNT_ARRAYS:
                v = np.asarray(st['solutions/solution_%d/%s' % (i, k)])
                assert v.shape == (4, K) and np.array_equal(v, on[i]['region_change_counts'][k]), (i, k)
    workflow.fit_model(exp_file, str(tmp_path / 'r0.store'), dict(config, cn_regions=cn_regions), None, seeds=seeds)
    with pipeline._Store(str(tmp_path / 'r0.store'), 'r') as st:
        assert not any('num_changes' in k or 'num_total_changes' in k for k in st.keys())


def test_size(hip):
    """2 000 segments x 165 states, 4 restarts, whole-chain queries with 16 bins: many steps, the saturating bin, and --
    with more queries than one chunk of the staging buffer holds -- more than one launch (timed, no time asserted).
    Over a chain of 400 segments the low bins are not representable beside the run's total, which the recursion is scaled
    by: measured on an MI355X, the bins come out as (-inf, ..., -inf, -592, -356, -132, -12.3, -4.4e-6), the bins below
    about 1e-308 of the total as -inf.  So no result may be NaN, the last bin is finite and the bins add up to 1."""
    from remixt_amd.restarts import RestartSet
    e = synthetic.make_experiment(2000, num_clones=3, max_copy_number=8, num_chains=5, seed=0)
    ps = synthetic.make_init_params(e, 4, 8)
    rs = RestartSet(e, ps, 8, num_clones=3, quiet=True, seeds=list(range(4)))
    try:
        rs.variational_update(1)
        b, m = rs.batch, rs.models[0]
        S = b.num_cn_states
        assert S == 165
        masks, labels = posteriors.event_tables(b.cn_classes)
        cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
        q = np.array([[a, z, -1, li] for a, z in zip(cs, ce) for li in (0, 1)], dtype=np.int32)
        b.profile_reset(); b.profile_enable(1)
        t0 = time.perf_counter()
        lp = b.region_counts_raw(0, 4, q, masks, labels, None, 16)
        wall = time.perf_counter() - t0
        ms, launches = b.profile()['k_region_counts']; b.profile_enable(0)
        print('whole chains, 4 restarts x %d queries x 16 bins over %d segments: %.1f ms wall, k_region_counts %.2f ms device in %d launches' % (
            len(q), b.num_segments, wall * 1e3, ms, launches))
        assert lp.shape == (4, len(q), 16) and not np.isnan(lp).any() and np.isfinite(lp[..., 15]).all()
        L = np.repeat(ce - cs + 1, 2)
        assert (np.abs(_lse(lp)) <= (L * (4 * S + 32) * U + 16 * U)[None]).all()
        assert L.max() > 300
        # chunking over queries: the same queries many times over, more than one chunk of the 64 MiB staging buffer holds
        reps = (64 << 20) // (4 * 16 * 8 + 16) // len(q) + 2
        short = np.array([[int(cs[0]), int(cs[0]) + 2, -1, 0], [int(cs[1]), int(cs[1]) + 20, -1, 1]], dtype=np.int32)
        many = np.tile(short, (reps * len(q) // 2, 1))
        b.profile_reset(); b.profile_enable(1)
        big = b.region_counts_raw(0, 4, many, masks, labels, None, 16)
        launches = b.profile()['k_region_counts'][1]; b.profile_enable(0)
        assert launches >= 2
        assert (big[:, 0::2] == big[:, :1]).all() and (big[:, 1::2] == big[:, 1:2]).all()
    finally:
        rs.close()
