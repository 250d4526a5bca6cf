"""Region event probabilities on the device (rmx_region_prob / k_region_prob): against the log-domain numpy twin on the
read-back framelogprob / log_transmat, the exact identities of the recursion, the adjacent joints, the sampler,
invariance to batching and grouping, no side effects on the model, errors, the pipeline, and the bench-size workload."""
import time

import numpy as np
import pytest

from remixt_amd import posteriors, synthetic
from tests import helpers as H
from tests import region_twin
from tests.test_hip_sample_cn import GRIDS, _fitted, _model_state, _pipeline_case, _same_results

pytestmark = pytest.mark.gpu

U = 2. ** -53
MASKS, LABELS = posteriors.MASK_NAMES, posteriors.LABEL_NAMES
# (mask, label) of every constraint a query is run with: none, each mask, each label, two of mask + label
CONSTRAINTS = [(None, None)] + [(k, None) for k in MASKS] + [(None, k) for k in LABELS] + [('not_loh', 'total'), ('not_subclonal', 'unphased')]


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


class Case(object):
    """A fitted model with everything the comparisons share: tables, per-segment masks / labels, the twin (built once)."""

    def __init__(self, m, batch=None, r=None, seg_is_original=None, is_telomere=None, breakpoint_idx=None):
        self.m = m
        self.b = m.model._batch if batch is None else batch
        self.r = m.model._r if r is None else r
        b = self.b
        self.N, self.S = b.num_segments, b.num_cn_states
        self.masks, self.labels = posteriors.event_tables(b.cn_classes)
        self.constrain = np.asarray(m.seg_is_original if seg_is_original is None else seg_is_original, dtype=bool)
        self.tel = np.asarray(m.is_telomere if is_telomere is None else is_telomere)
        self.bidx = np.asarray(m.breakpoint_idx if breakpoint_idx is None else breakpoint_idx)
        self.cs, self.ce = posteriors.chains_from_telomeres(self.tel)
        self.mask_seg = dict((k, self.masks[b.seg_class, i].astype(bool)) for i, k in enumerate(MASKS))
        self.label_seg = dict((k, self.labels[b.seg_class, i]) for i, k in enumerate(LABELS))
        self.twin = region_twin.RegionTwin(b.get_array(self.r, 'framelogprob'), b.get_array(self.r, 'log_transmat'), self.cs, self.ce)

    def queries(self):
        """(a, b) runs: one segment, two over a plain and over a breakend adjacency, a whole chain, a run from a chain start
        and one to a chain end."""
        inner = np.ones(self.N - 1, dtype=bool); inner[self.ce[:-1]] = False
        plain = np.flatnonzero(inner & (self.bidx[:-1] < 0))
        be = np.flatnonzero(inner & (self.bidx[:-1] >= 0))
        assert len(plain) and len(be), 'the case needs plain and breakend adjacencies'
        c = int(np.argmax(self.ce - self.cs))
        mid = int(plain[len(plain) // 2])
        return [(mid, mid), (mid, mid + 1), (int(be[0]), int(be[0]) + 1), (int(be[-1]), int(be[-1]) + 1), (int(self.cs[c]), int(self.ce[c])),
                (int(self.cs[1]), int(min(self.cs[1] + 3, self.ce[1]))), (int(max(self.ce[0] - 2, self.cs[0])), int(self.ce[0]))]

    def raw(self, runs, constraints=CONSTRAINTS, r0=None, nr=1):
        q = np.array([[a, b, -1 if mk is None else MASKS.index(mk), -1 if lb is None else LABELS.index(lb)]
                      for (a, b) in runs for (mk, lb) in constraints], dtype=np.int32)
        out = self.b.region_logprob_raw(self.r if r0 is None else r0, nr, q, self.masks, self.labels, self.constrain)
        return out.reshape(nr, len(runs), len(constraints))

    def want(self, a, b, mk, lb):
        return self.twin.logprob(a, b, None if mk is None else self.mask_seg[mk], None if lb is None else self.label_seg[lb], self.constrain)

    def check_against_twin(self, runs, constraints=CONSTRAINTS, tag=''):
        got = self.raw(runs, constraints)[0]
        worst = 0.
        for i, (a, b) in enumerate(runs):
            L = b - a + 1
            for j, (mk, lb) in enumerate(constraints):
                want = self.want(a, b, mk, lb)
                err = abs(np.exp(got[i, j]) - np.exp(want))
                worst = max(worst, err / L)
                print('%s run [%d, %d] mask %s label %s: log P %.17g (twin %.17g), |P - twin| %.3e' % (tag, a, b, mk, lb, got[i, j], want, err))
                assert err <= L * 1e-9, (tag, a, b, mk, lb, got[i, j], want)
                if mk is None and lb is None:
                    assert abs(got[i, j]) <= L * (4 * self.S + 32) * U, (tag, a, b, got[i, j])
        print('%s worst |P - twin| / L: %.3e' % (tag, worst))
        return got


@pytest.fixture(scope='module')
def cases(hip):
    return dict(((N, M, c), Case(_fitted(hip, N, M, c))) for N, M, c in GRIDS)


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_twin(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    assert case.S == {8: 165, 12: 355, 6: 457}[max_cn] and case.S % 64
    assert case.m.num_breakpoints > 0 and (case.bidx >= 0).any()
    b = case.b
    b.profile_reset(); b.profile_enable(1)
    got = case.check_against_twin(case.queries(), tag='S %d' % case.S)
    prof = b.profile(); b.profile_enable(0)
    assert prof['k_region_prob'][1] == 1 and prof['k_region_prob'][0] > 0
    assert np.isfinite(got[:, 0]).all() and (got <= (4 * case.S + 32) * U * N).all()
    # the model-level form
    q = np.array([[a, b_, 0, 1] for a, b_ in case.queries()], dtype=np.int32)
    one = case.m.model.region_logprob(q, case.masks, case.labels, case.constrain)
    assert one.shape == (len(q),) and np.array_equal(one, b.region_logprob_raw(case.r, 1, q, case.masks, case.labels, case.constrain)[0])


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_identities(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    b, S = case.b, case.S
    # every unconstrained run has probability 1: every pair of segments of the longest chain
    c = int(np.argmax(case.ce - case.cs))
    seg = np.arange(case.cs[c], case.ce[c] + 1)
    runs = [(int(a), int(e)) for a in seg for e in seg if a <= e]
    got = case.raw(runs, [(None, None)])[0, :, 0]
    for (a, e), lp in zip(runs, got):
        assert abs(lp) <= (e - a + 1) * (4 * S + 32) * U, (a, e, lp)
    print('S %d unconstrained: max |log P| %.3e over %d runs (bound per segment %.3e)' % (S, np.abs(got).max(), len(runs), (4 * S + 32) * U))
    # a one-segment mask query is the mask's sum of the marginals; without constrain the mask binds the inserted segments too
    post = b.get_array(case.r, 'posterior_marginals')
    for constrain in (case.constrain, None):
        q = np.array([[n, n, i, -1] for n in range(case.N) for i in range(len(MASKS))], dtype=np.int32)
        lp = b.region_logprob_raw(case.r, 1, q, case.masks, None, constrain)[0].reshape(case.N, len(MASKS))
        for i, k in enumerate(MASKS):
            want = np.where(case.mask_seg[k], post, 0.).sum(axis=1)
            if constrain is not None:
                want = np.where(constrain, want, post.sum(axis=1))
            with np.errstate(divide='ignore'):
                assert np.array_equal(lp[:, i] == -np.inf, want == 0), k
            ok = want > 0
            # (S + 4) 2^-53 relative for the sum itself, and what a float64 logarithm can carry at all: log P is rounded
            # (half an ulp, 2^-53 |log P|) after a library log of at most an ulp, and an error d of log P is a relative
            # error d of P.  Where P is not tiny the second term vanishes beside the first.
            tol = ((S + 4) + 3 * np.abs(np.log(want[ok]))) * U
            rel = np.abs(np.exp(lp[ok, i]) / want[ok] - 1)
            assert (rel <= tol).all(), (k, rel.max())
    assert (lp[:, MASKS.index('hdel')] == -np.inf).all()      # (a normal row of (1, 1): no state is a homozygous deletion)


def test_inserted_segments(hip):
    """Two breakends on one boundary: the model inserts a zero-length segment there.  A mask does not bind it, a label
    constraint binds the adjacencies through it, and the public forms map experiment segments onto the runs."""
    e = synthetic.make_experiment(60, num_clones=3, max_copy_number=4, num_chains=3, seed=7)
    e.breakpoints = H.add_shared_boundary_breakpoints(e)
    m, h, _ = H.make_model(hip, M=3, max_cn=4, experiment=e)
    H.attach(m, h)
    m.variational_update(); m.variational_update()
    case = Case(m)
    assert m.N1 > m.N and not case.constrain.all()
    dummy = int(np.flatnonzero(~case.constrain & (np.arange(m.N1) > 0) & (case.tel == 0))[0])
    assert case.constrain[dummy - 1] and case.constrain[dummy + 1]
    case.check_against_twin([(dummy - 1, dummy + 1), (dummy, dummy), (dummy, dummy + 1)], tag='inserted segment')
    lp = case.raw([(dummy, dummy)], [(k, None) for k in MASKS])[0, 0]
    assert (np.abs(lp) <= (case.S + 4) * U).all()                      # no mask binds the inserted segment, 'hdel' included
    # the experiment pair around it, through region_events: the run holds the inserted segment
    i = int(m.seg_rev_remap[dummy - 1])
    assert m.seg_fwd_remap[i] == dummy - 1 and m.seg_fwd_remap[i + 1] == dummy + 1
    ev = m.region_events([(i, i + 1), (i, i)])
    for name, mk, lb, complement in posteriors.REGION_EVENTS:
        for j, (a, b) in enumerate(((dummy - 1, dummy + 1), (dummy - 1, dummy - 1))):
            want = np.exp(case.want(a, b, mk, lb))
            assert abs(ev[name][j] - (1. - want if complement else want)) <= 3e-9, (name, j)
    assert abs(m.cn_change_prob()[i] - (1. - ev['p_no_change'][0])) <= 1e-15


def test_against_the_joint(hip, cases):
    case = cases[GRIDS[0]]
    joint = case.b.get_array(case.r, 'joint_posterior_marginals')
    inner = np.ones(case.N - 1, dtype=bool); inner[case.ce[:-1]] = False
    ns = np.flatnonzero(inner)
    plain = case.bidx[ns] < 0
    assert plain.any() and (~plain).any()
    got = case.raw([(int(n), int(n) + 1) for n in ns], [(None, 'state')])[0, :, 0]
    want = np.trace(joint[ns], axis1=1, axis2=2)
    err = np.abs(np.exp(got) - want)
    print('state-label pairs against trace(joint): max err %.3e (plain %.3e, breakend %.3e)' % (err.max(), err[plain].max(), err[~plain].max()))
    assert (err <= 1e-9).all()
    # the same through the public form, in experiment order
    change = case.m.cn_change_prob()
    regs, n = posteriors.adjacency_regions(case.m.seg_fwd_remap, case.m.is_telomere)
    assert change.shape == (case.m.N - 1,) and np.array_equal(np.isnan(change), ~np.isin(np.arange(case.m.N - 1), n))
    direct = [i for i in n if case.m.seg_fwd_remap[i + 1] == case.m.seg_fwd_remap[i] + 1]
    assert len(direct) > 10
    for i in direct:
        assert abs(change[i] - (1. - np.trace(joint[case.m.seg_fwd_remap[i]]))) <= 1e-9


def test_against_the_sampler(hip):
    from tests.test_hip_posterior_summary import _fitted as fitted_masked
    m = fitted_masked(hip, 30, 3, 8, sweeps=3, masked=True)      # (read counts masked out: events of intermediate probability)
    case = Case(m)
    K = 4096
    st = case.b.sample_states(case.r, 1, K, [99]).astype(np.int64)[0]
    runs = case.queries()
    got = np.exp(case.raw(runs)[0])
    informative = 0
    for i, (a, e) in enumerate(runs):
        seg = np.arange(a, e + 1)
        for j, (mk, lb) in enumerate(CONSTRAINTS):
            hit = np.ones(K, dtype=bool)
            if mk is not None:
                for n in seg[case.constrain[seg]]:
                    hit &= case.mask_seg[mk][n, st[:, n]]
            if lb is not None:
                for n in seg[:-1]:
                    hit &= case.label_seg[lb][n, st[:, n]] == case.label_seg[lb][n + 1, st[:, n + 1]]
            P = got[i, j]
            tol = 6 * np.sqrt(P * (1 - min(P, 1.)) / K) + 2. / K
            informative += 0.01 < P < 0.99
            assert abs(hit.mean() - P) <= tol, (a, e, mk, lb, hit.mean(), P)
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
        # (the allele likelihood of an LOH state under normal contamination is the reference's ValueError 'p <= 0 or (1 - p) <= 0',
        # and a normal row of (1, 0) makes such states: the sweeps run on the total read counts alone)
        b.set_array(0, 'allele_likelihood_mask', np.zeros(N, dtype=np.int64))
        b.variational_update(2)
        case = Case(m, batch=b, r=0)
        loh = case.masks[:, MASKS.index('loh')]
        assert not loh[0].any() and loh[1].any()                         # the mask differs per class
        assert np.array_equal(case.labels[0], case.labels[1])            # the tumour copies do not
        got = case.check_against_twin(case.queries(), tag='two classes')
        # (a kernel that took class 0's masks everywhere would call LOH impossible)
        runs = [(n, n) for n in range(1, N, 2)]
        lp = case.raw(runs, [('loh', None)])[0, :, 0]
        assert (lp[case.constrain[1::2]] > -np.inf).any()
        assert (case.raw([(n, n) for n in range(0, N, 2)], [('loh', None)])[0, :, 0][case.constrain[0::2]] == -np.inf).all()
        assert got.shape == (7, len(CONSTRAINTS))
    finally:
        b.close()


def test_mixed_transition_model(hip):
    """The snapshot of the last update_p_cn under another transition_model than the current one: the plain weights come
    from the snapshot model's log table, not from the current model's exp tables."""
    m = _fitted(hip, 40, 3, 4, seed=3)
    T0 = np.array(m.model.log_transmat)
    m.model.transition_model = 1
    assert np.array_equal(np.array(m.model.log_transmat), T0)            # the snapshot stays the model-0 one
    case = Case(m)
    case.check_against_twin(case.queries(), tag='mixed model')
    # the other way round
    m2 = _fitted(hip, 40, 3, 4, seed=3, transition_model=1)
    assert m2.model.transition_model == 1
    m2.model.transition_model = 0
    case2 = Case(m2)
    assert not np.array_equal(np.array(m2.model.log_transmat), T0)
    case2.check_against_twin(case2.queries()[:5], CONSTRAINTS[:1] + CONSTRAINTS[7:], tag='mixed model 1 -> 0')


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
    q = np.array([[a, e_, mi, li] for a, e_ in runs for mi, li in ((-1, -1), (1, -1), (-1, 1), (5, 2))], dtype=np.int32)
    full = b.region_logprob_raw(0, 4, q, masks, labels, constrain)
    assert full.shape == (4, len(q)) and not np.array_equal(full[0], full[1])
    for r in range(4):
        assert np.array_equal(b.region_logprob_raw(r, 1, q, masks, labels, constrain)[0], full[r], equal_nan=True)
    assert np.array_equal(b.region_logprob_raw(1, 2, q, masks, labels, constrain), full[1:3], equal_nan=True)
    for i in range(0, len(q), 5):
        assert np.array_equal(b.region_logprob_raw(0, 4, q[i:i + 1], masks, labels, constrain)[:, 0], full[:, i], equal_nan=True)
    assert np.array_equal(b.region_logprob_raw(0, 4, q[::-1].copy(), masks, labels, constrain), full[:, ::-1], equal_nan=True)
    per_set = rs.region_events(regions)
    change_set = rs.cn_change_prob()
    one = rs.models[2].region_events(regions)
    for k in posteriors.REGION_ARRAYS:
        assert per_set[k].shape == (4, len(regions)) and np.array_equal(per_set[k][2], one[k]), k
        assert ((per_set[k] >= 0) & (per_set[k] <= 1)).all(), k
    assert np.array_equal(change_set[2], rs.models[2].cn_change_prob(), equal_nan=True)
    rs.close()
    groups = RestartGroups(e, ps, 4, groups=2, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    single = RestartGroups(e, ps, 4, groups=1, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    for g in (groups, single):
        g.variational_update(2)
    a, c = groups.region_events(regions), single.region_events(regions)
    for k in posteriors.REGION_ARRAYS:
        assert a[k].shape == (4, len(regions)) and np.array_equal(a[k], c[k]), k
    assert np.array_equal(groups.cn_change_prob(), single.cn_change_prob(), equal_nan=True)
    groups.close(); single.close()


def test_no_side_effects(hip):
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    before = _model_state(m1)
    ev = m1.region_events([(0, 10), (5, 5), (20, 49)])
    ch = m1.cn_change_prob()
    assert set(ev) == set(posteriors.REGION_ARRAYS) and ch.shape == (m1.N - 1,)
    after = _model_state(m1)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    # a fit continued after the call equals one without it
    for m in (m1, m2):
        m.variational_update()
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
        b.region_logprob_raw(r, 1, ok, masks, labels)
    assert bpmodel.last_error_restarts() == [r]
    with pytest.raises(ValueError, match='update_p_cn'):
        m.region_events([(0, 3)])
    m.variational_update()
    N = b.num_segments
    bad = [([[3, 2, -1, -1]], 'first <= last'), ([[-1, 2, -1, -1]], 'first <= last'), ([[0, N, -1, -1]], 'first <= last'),
           ([[int(ce[0]), int(ce[0]) + 1, -1, -1]], 'chain end'), ([[int(cs[0]), int(ce[1]), -1, -1]], 'chain end'),
           ([[0, 1, len(MASKS), -1]], 'mask index'), ([[0, 1, -2, -1]], 'mask index'), ([[0, 1, -1, len(LABELS)]], 'label index'),
           ([[0, 1, -1, -2]], 'label index')]
    for q, text in bad:
        with pytest.raises(ValueError, match='^bad argument: .*' + text):
            b.region_logprob_raw(r, 1, ok + q, masks, labels)
        assert bpmodel.last_error_restarts() == []
    with pytest.raises(ValueError, match='^bad argument: .*mask index'):      # an index without a table
        b.region_logprob_raw(r, 1, ok, None, labels)
    for args in ((r + 1, 1), (-1, 1), (r, 0)):
        with pytest.raises(ValueError, match='^bad argument: bad restart range$'):
            b.region_logprob_raw(args[0], args[1], ok, masks, labels)
    with pytest.raises(ValueError, match='^bad argument: .*no queries'):
        b.region_logprob_raw(r, 1, np.zeros((0, 4), dtype=np.int32), masks, labels)
    for kw in (dict(queries=[[0, 1, 0]]), dict(masks=masks[:, :, :-1]), dict(labels=labels[:1, :, :-1]), dict(constrain=np.ones(N + 1))):
        args = dict(queries=ok, masks=masks, labels=labels, constrain=None); args.update(kw)
        with pytest.raises(ValueError, match='must have shape'):
            b.region_logprob_raw(r, 1, **args)
    with pytest.raises(ValueError):
        m.region_events([(4, 2)])
    assert b.region_logprob_raw(r, 1, ok, masks, labels).shape == (1, 1)
    from oracle import oracle
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError):
        mo.region_events([(0, 3)])
    with pytest.raises(NotImplementedError):
        mo.cn_change_prob()


def test_pipeline_cn_regions(hip, tmp_path):
    from remixt_amd import workflow
    from remixt_amd.analysis import pipeline
    from remixt_amd.restarts import RestartSet
    import pickle
    e, config, init_params = _pipeline_case()
    ids = sorted(init_params)
    seeds = [100 + i for i in ids]
    cn_regions = [('geneA', 10, 14), ('arm', 0, 250), ('seg', 77, 77), ('pair', 300, 301)]
    base = pipeline.fit_restarts(e, init_params, config, seeds=seeds, groups=1)
    on = pipeline.fit_restarts(e, init_params, dict(config, cn_regions=cn_regions), seeds=seeds, groups=1)
    # unset: nothing of it in the results; set: the same results plus region_events
    assert not any('region_events' in res for res in base.values())
    _same_results(base, dict((i, dict((k, v) for k, v in res.items() if k != 'region_events')) for i, res in on.items()))
    # recomputation from the same fit
    rs = RestartSet(e, [init_params[i] for i in ids], 4, num_clones=3, quiet=True, seeds=seeds, **pipeline._model_kwargs(e, config))
    rs.fit(config['num_em_iter'], config['num_update_iter'])
    want = rs.region_events([(a, b) for _, a, b in cn_regions])
    rs.close()
    for j, i in enumerate(ids):
        ev = on[i]['region_events']
        assert ev['names'] == ['geneA', 'arm', 'seg', 'pair'] and sorted(ev) == sorted(posteriors.REGION_ARRAYS + ('names',))
        for k in posteriors.REGION_ARRAYS:
            assert ev[k].shape == (4,) and ((ev[k] >= 0) & (ev[k] <= 1)).all() and np.array_equal(ev[k], want[k][j]), (i, k)
        assert (ev['p_all_loh'] <= ev['p_any_loh'] + 1e-12).all() and (ev['p_no_change'] <= ev['p_no_total_change'] + 1e-12).all()
        assert abs(ev['p_no_change'][2] - 1.) <= 1e-12 and abs(ev['p_all_loh'][2] - ev['p_any_loh'][2]) <= 1e-12      # one segment
    one = pipeline.fit(e, init_params[ids[1]], dict(config, cn_regions=cn_regions), quiet=True, init_id=ids[1])
    assert one['region_events']['names'] == on[ids[1]]['region_events']['names'] and one['region_events']['p_no_change'].shape == (4,)
    # the workflow (fit_restarts_distributed + collate): the arrays in the record and in the store
    exp_file = str(tmp_path / 'experiment.pickle')
    with open(exp_file, 'wb') as f:
        pickle.dump(e, f)
    workflow.fit_model(exp_file, str(tmp_path / 'r.store'), dict(config, cn_regions=cn_regions), None)
    with pipeline._Store(str(tmp_path / 'r.store'), 'r') as st:
        for i in sorted(st['stats']['init_id']):
            assert list(st['solutions/solution_%d/region_names' % i]) == ['geneA', 'arm', 'seg', 'pair']
            for k in posteriors.REGION_ARRAYS:
                v = np.asarray(st['solutions/solution_%d/%s' % (i, k)])
                assert v.shape == (4,) and ((v >= 0) & (v <= 1)).all(), (i, k)
    workflow.fit_model(exp_file, str(tmp_path / 'r0.store'), config, None)
    with pipeline._Store(str(tmp_path / 'r0.store'), 'r') as st:
        assert not any('region_names' in k or 'p_no_change' in k for k in st.keys())


def test_full_size(hip):
    """50 000 segments, 165 states, 16 restarts: every adjacency through cn_change_prob (timed, no time asserted)."""
    from remixt_amd.restarts import RestartSet
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=8, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, 16, 8)
    rs = RestartSet(e, ps, 8, num_clones=3, quiet=True, seeds=list(range(16)))
    try:
        rs.variational_update(1)
        b, m = rs.batch, rs.models[0]
        assert b.num_cn_states == 165
        rs.cn_change_prob()
        b.profile_reset(); b.profile_enable(1)
        t0 = time.perf_counter()
        change = rs.cn_change_prob()
        wall = time.perf_counter() - t0
        ms, launches = b.profile()['k_region_prob']; b.profile_enable(0)
        print('cn_change_prob, 16 restarts x %d adjacencies: %.1f ms wall, k_region_prob %.2f ms device in %d launches' % (
            change.shape[1], wall * 1e3, ms, launches))
        N = len(e.l)
        assert change.shape == (16, N - 1)
        joined = np.zeros(N - 1, dtype=bool); joined[[a for a, _ in e.adjacencies]] = True
        assert np.array_equal(np.isnan(change), np.broadcast_to(~joined, change.shape))
        assert (change[:, joined] >= 0).all() and (change[:, joined] <= 1).all()
        # restart 1 against the adjacent joints at 200 adjacencies whose two segments are neighbours in the model
        fwd = m.seg_fwd_remap
        direct = np.flatnonzero(joined & (fwd[1:] == fwd[:-1] + 1))
        pick = np.random.RandomState(0).choice(direct, size=200, replace=False)
        joint = b.get_array(1, 'joint_posterior_marginals')
        for i in pick:
            assert abs(change[1, i] - (1. - np.trace(joint[fwd[i]]))) <= 1e-9, i
        del joint
    finally:
        rs.close()
