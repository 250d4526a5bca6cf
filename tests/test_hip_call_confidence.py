"""Call probabilities on the device (rmx_call_prob / k_call_prob): against the log-domain numpy twin on the read-back
framelogprob / log_transmat, the exact identities of the recursion, the reduction to rmx_region_prob, the sampler,
inserted segments, two state classes, the mixed transition model, invariance to batching and grouping, no side effects
on the model, errors, the pipeline, and the bench-size workload.

Measured on an MI355X (printed by test_against_twin): worst |P - twin| / L 1.1e-16, 1.1e-16, 2.2e-16 and worst
|log P - twin| / L 7.1e-16, 3.6e-15, 8.9e-16 at 165, 355 and 457 states, against the budget of 1e-9 for both."""
import ctypes as C
import time

import numpy as np
import pytest

from remixt_amd import posteriors, synthetic
from tests import call_twin
from tests import helpers as H
from tests.test_hip_region_events import Case
from tests.test_hip_sample_cn import GRIDS, _fitted, _model_state, _pipeline_case, _same_results

pytestmark = pytest.mark.gpu

U = 2. ** -53
LABELS = posteriors.LABEL_NAMES
# the label of a query: -1 (the state itself) and the three tables
QLABELS = [None, 'state', 'unphased', 'total']


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


def _li(lb):
    return -1 if lb is None else LABELS.index(lb)


def _decoded(b, r):
    cn, _ = b.infer_cn_batch(r, 1)
    return posteriors.cn_to_states(cn[0], b.cn_classes, b.seg_class)


def _paths(case):
    """D: the decoded path; A: the marginal arg-max path; X: A with every fifth segment at the runner-up of its marginal."""
    post = case.b.get_array(case.r, 'posterior_marginals')
    order = np.argsort(post, axis=1, kind='stable')
    A = order[:, -1].astype(np.int16)
    X = A.copy(); X[::5] = order[::5, -2]
    return np.stack([_decoded(case.b, case.r), A, X]), post


def _raw(case, paths, runs, labels=QLABELS, constrain='default', tab=None):
    """(len(paths), len(runs), len(labels)) log-probabilities from one device call."""
    q = np.array([[a, e, _li(lb), p] for p in range(len(paths)) for (a, e) in runs for lb in labels], dtype=np.int32)
    cs = case.constrain if isinstance(constrain, str) else constrain
    out = case.b.call_logprob_raw(case.r, 1, np.asarray(paths)[None], q, case.labels if tab is None else tab, cs)
    return out[0].reshape(len(paths), len(runs), len(labels))


def _want(case, a, e, lb, path, constrain='default'):
    cs = case.constrain if isinstance(constrain, str) else constrain
    return call_twin.logprob(case.twin, a, e, None if lb is None else case.label_seg[lb], path, cs)


def _check_against_twin(case, paths, runs, labels=QLABELS, constrain='default', tag=''):
    got = _raw(case, paths, runs, labels, constrain)
    worst_p = worst_log = 0.
    for p, path in enumerate(paths):
        for i, (a, e) in enumerate(runs):
            L = e - a + 1
            for j, lb in enumerate(labels):
                want = _want(case, a, e, lb, path, constrain)
                err = abs(np.exp(got[p, i, j]) - np.exp(want))
                worst_p = max(worst_p, err / L)
                assert err <= L * 1e-9, (tag, p, a, e, lb, got[p, i, j], want)
                if want > -300:
                    lerr = abs(got[p, i, j] - want)
                    worst_log = max(worst_log, lerr / L)
                    print('%s path %d run [%d, %d] label %s: log P %.17g (twin %.17g), |log P - twin| %.3e' % (tag, p, a, e, lb, got[p, i, j], want, lerr))
                    assert lerr <= L * 1e-9, (tag, p, a, e, lb, got[p, i, j], want)
    print('%s worst |P - twin| / L: %.3e, worst |log P - twin| / L: %.3e' % (tag, worst_p, worst_log))
    return got


@pytest.fixture(scope='module')
def cases(hip):
    return dict(((N, M, c), Case(_fitted(hip, N, M, c))) for N, M, c in GRIDS)


@pytest.fixture(scope='module')
def masked(hip):
    from tests.test_hip_posterior_summary import _fitted as fitted_masked
    return Case(fitted_masked(hip, 30, 3, 8, sweeps=3, masked=True))      # (read counts masked out: events of intermediate probability)


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_twin(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    assert case.S == {8: 165, 12: 355, 6: 457}[max_cn] and case.S % 64
    assert case.m.num_breakpoints > 0 and (case.bidx >= 0).any()
    paths, _ = _paths(case)
    b = case.b
    b.profile_reset(); b.profile_enable(1)
    got = _check_against_twin(case, paths, case.queries(), tag='S %d' % case.S)
    prof = b.profile(); b.profile_enable(0)
    assert prof['k_call_prob'][1] == 1 and prof['k_call_prob'][0] > 0
    assert not np.isnan(got).any() and (got <= (4 * case.S + 32) * U * N).all()
    assert (got[2] < -5).any()                                           # (X is an unlikely path: the test is not all P = 1)
    # (d) label -1 and label 'state' name the same sets
    assert np.array_equal(got[:, :, 0], got[:, :, 1])
    # (e) set inclusion
    for i, (a, e) in enumerate(case.queries()):
        tol = (e - a + 1) * (4 * case.S + 32) * U
        assert (got[:, i, 1] <= got[:, i, 2] + tol).all() and (got[:, i, 2] <= got[:, i, 3] + tol).all(), (a, e)
    # the model-level form
    q = np.array([[a, e, LABELS.index('total'), 1] for a, e in case.queries()], dtype=np.int32)
    one = case.m.model.call_logprob(paths, q, case.labels, case.constrain)
    assert one.shape == (len(q),) and np.array_equal(one, got[1, :, 3])


def test_against_twin_masked(hip, masked):
    case = masked
    D = _decoded(case.b, case.r)
    smp = case.b.sample_states(case.r, 1, 8, [5])[0]
    got = _check_against_twin(case, np.concatenate([D[None], smp]), case.queries(), tag='masked fit')
    P = np.exp(got[0])
    assert ((P > 0.001) & (P < 0.999)).sum() >= 3


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_identities(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    b, S = case.b, case.S
    paths, post = _paths(case)
    seg = [(n, n) for n in range(case.N)]
    everywhere = np.ones(case.N, dtype=bool)
    got = _raw(case, paths, seg, constrain=everywhere)                    # (3, N, 4)
    for p, path in enumerate(paths):
        summary = b.posterior_summary_raw(case.r, 1, states=path[None].astype(np.int64))[1][0, :, 2]
        for j, lb in enumerate(QLABELS):
            # (a) the marginal at the reference state; (b) the label set's sum of the marginals
            mask = call_twin.call_mask(None if lb is None else case.label_seg[lb], path, S)
            want = np.where(mask, post, 0.).sum(axis=1)
            if lb is None:
                assert np.array_equal(want, post[np.arange(case.N), path])
            assert np.array_equal(got[p, :, j] == -np.inf, want == 0), (p, lb)
            ok = want > 0
            tol = ((S + 4) + 3 * np.abs(np.log(want[ok]))) * U
            rel = np.abs(np.exp(got[p, ok, j]) / want[ok] - 1)
            assert (rel <= tol).all(), (p, lb, rel.max())
            if lb is None:
                assert np.array_equal(summary == 0, want == 0)
                assert (np.abs(np.exp(got[p, ok, j]) / summary[ok] - 1) <= tol).all(), p
    # (c) an unbound segment alone
    free = _raw(case, paths, seg, constrain=np.zeros(case.N, dtype=bool))
    assert (np.abs(free) <= (S + 4) * U).all(), np.abs(free).max()
    print('S %d: unbound single segments, max |log P| %.3e (bound %.3e)' % (S, np.abs(free).max(), (S + 4) * U))
    # (f) a constant reference state over a run with every segment bound: rmx_region_prob with the mask of its label
    assert b.cn_classes.shape[0] == 1
    worst = 0.
    for a, e in case.queries():
        s0 = int(paths[0][a])
        const = np.full((1, case.N), s0, dtype=np.int16)
        for li, lb in enumerate(LABELS):
            mask = (case.labels[:, li] == case.labels[:, li, s0][:, None])[:, None, :].astype(np.uint8)      # (C, 1, S)
            want = b.region_logprob_raw(case.r, 1, [[a, e, 0, -1]], mask, None, None)[0, 0]
            have = _raw(case, const, [(a, e)], [lb], constrain=None)[0, 0, 0]
            tol = (e - a + 1) * (4 * S + 32) * U
            if want == -np.inf or have == -np.inf:
                assert want == have, (a, e, lb)
                continue
            worst = max(worst, abs(have - want) / tol)
            assert abs(have - want) <= tol, (a, e, lb, have, want)
    print('S %d: against k_region_prob with a one-label mask, worst error / bound %.3f' % (S, worst))


def test_decoded_path_is_the_mode(hip, masked):
    case = masked
    D = _decoded(case.b, case.r)
    smp = case.b.sample_states(case.r, 1, 64, [7])[0]
    chains = [(int(a), int(e)) for a, e in zip(case.cs, case.ce)]
    got = _raw(case, np.concatenate([D[None], smp]), chains, [None], constrain=None)[:, :, 0]      # (65, chains)
    assert np.isfinite(got).all()
    assert (got[0][None] >= got[1:] - case.N * 1e-9).all()
    assert (got[0][None] > got[1:] + 1e-6).any()
    print('log q of the decoded path per chain %s; best sample %s' % (got[0], got[1:].max(axis=0)))


def test_against_the_sampler(hip, masked):
    case = masked
    K = 4096
    st = case.b.sample_states(case.r, 1, K, [99]).astype(np.int64)[0]
    D = _decoded(case.b, case.r)
    refs = np.stack([D, st[0].astype(np.int16)])
    runs = [(int(a), int(e)) for a, e in zip(case.cs, case.ce)]
    for c0, c1 in zip(case.cs, case.ce):
        for L in (1, 3, 10):
            for a in range(int(c0), int(c1) - L + 2, max(1, L // 2)):
                runs.append((a, a + L - 1))
    got = np.exp(_raw(case, refs, runs))
    informative = 0
    for p, ref in enumerate(refs):
        for i, (a, e) in enumerate(runs):
            seg = np.arange(a, e + 1)
            seg = seg[case.constrain[seg]]
            for j, lb in enumerate(QLABELS):
                hit = np.ones(K, dtype=bool)
                for n in seg:
                    if lb is None:
                        hit &= st[:, n] == ref[n]
                    else:
                        hit &= case.label_seg[lb][n, st[:, n]] == case.label_seg[lb][n, ref[n]]
                P = got[p, i, j]
                tol = 6 * np.sqrt(P * (1 - min(P, 1.)) / K) + 2. / K
                informative += 0.01 < P < 0.99
                assert abs(hit.mean() - P) <= tol, (p, a, e, lb, hit.mean(), P)
    print('against the sampler: %d events, %d with 0.01 < P < 0.99' % (got.size, informative))
    assert informative >= 3


def test_inserted_segments(hip):
    """Two breakends on one boundary: the model inserts a zero-length segment there.  The call does not bind it: it is
    marginalised, whatever the reference path holds there."""
    e = synthetic.make_experiment(60, num_clones=3, max_copy_number=4, num_chains=3, seed=7)
    e.breakpoints = H.add_shared_boundary_breakpoints(e)
    m, h, _ = H.make_model(hip, M=3, max_cn=4, experiment=e)
    H.attach(m, h)
    m.variational_update(); m.variational_update()
    case = Case(m)
    assert m.N1 > m.N and not case.constrain.all()
    dummy = int(np.flatnonzero(~case.constrain & (np.arange(m.N1) > 0) & (case.tel == 0))[0])
    assert case.constrain[dummy - 1] and case.constrain[dummy + 1]
    paths, post = _paths(case)
    other = paths.copy()
    other[:, dummy] = [s for s in np.argsort(post[dummy])[::-1] if s not in set(paths[:, dummy])][0]      # another state at the inserted segment
    assert (other[:, dummy] != paths[:, dummy]).all()
    runs = [(dummy - 1, dummy + 1), (dummy, dummy), (dummy, dummy + 1), (dummy - 1, dummy)]
    got = _check_against_twin(case, paths, runs, tag='inserted segment')
    assert np.array_equal(got, _raw(case, other, runs))                  # bit for bit
    assert (np.abs(got[:, 1]) <= (case.S + 4) * U).all()                 # the inserted segment alone
    # with every segment bound it depends on what the path holds there
    bound = _check_against_twin(case, paths, runs, constrain=None, tag='inserted segment bound')
    bound_other = _check_against_twin(case, other, runs, constrain=None, tag='inserted segment bound, third state')
    assert not np.array_equal(bound, bound_other) and (bound[:, 0] <= got[:, 0] + 3 * (4 * case.S + 32) * U).all() and (bound_other[:, 0] < got[:, 0]).all()
    # the public forms, for the decoded path: the experiment pair around the inserted segment holds it
    i = int(m.seg_rev_remap[dummy - 1])
    assert m.seg_fwd_remap[i] == dummy - 1 and m.seg_fwd_remap[i + 1] == dummy + 1
    conf = m.call_confidence([(i, i + 1), (i, i)])
    D = paths[0]
    assert sorted(conf) == sorted(posteriors.CALL_ARRAYS)
    for name, lb in posteriors.CALL_LABELS:
        for j, (a, b_) in enumerate(((dummy - 1, dummy + 1), (dummy - 1, dummy - 1))):
            want = np.exp(_want(case, a, b_, lb, D))
            assert conf[name].shape == (2,) and abs(conf[name][j] - want) <= 3e-9, (name, j)
    want = sum(_want(case, int(a), int(b_), None, D) for a, b_ in zip(case.cs, case.ce))
    lq = m.cn_logprob()
    print('cn_logprob of the decoded path %.17g (twin %.17g)' % (lq, want))
    assert isinstance(lq, float) and abs(lq - want) <= case.N * 1e-9
    # a call handed over in experiment order: the decoded path again, and two paths at once
    cn, _ = m.optimal_cn()
    assert m.cn_logprob(cn) == lq and np.array_equal(m.call_confidence([(i, i + 1)], cn)['p_call'], conf['p_call'][:1])
    cnX = case.b.states_to_cn(paths[2])[m.seg_fwd_remap]
    two = m.cn_logprob(np.stack([cn, cnX]))
    assert two.shape == (2,) and two[0] == lq and two[1] < lq
    assert abs(two[1] - sum(_want(case, int(a), int(b_), None, paths[2]) for a, b_ in zip(case.cs, case.ce))) <= case.N * 1e-9


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
        # (see test_two_classes of test_hip_region_events: the sweeps run on the total read counts alone)
        b.set_array(0, 'allele_likelihood_mask', np.zeros(N, dtype=np.int64))
        b.variational_update(2)
        case = Case(m, batch=b, r=0)
        # the event tables label the tumour copies, which the classes share: a table that differs per class instead --
        # class 0 by the totals, class 1 up to the phase
        tab = np.stack([case.labels[0, [LABELS.index('total')]], case.labels[1, [LABELS.index('unphased')]]])      # (2, 1, S)
        assert not np.array_equal(tab[0], tab[1])
        lab_seg = tab[seg_class, 0]
        paths, _ = _paths(case)
        runs = case.queries() + [(n, n) for n in range(1, N, 2)]
        q = np.array([[a, e_, 0, p] for p in range(3) for a, e_ in runs], dtype=np.int32)
        got = b.call_logprob_raw(0, 1, paths[None], q, tab, case.constrain)[0].reshape(3, len(runs))
        wrong_lab = np.broadcast_to(tab[0, 0], lab_seg.shape)             # what a kernel that took class 0's labels everywhere would see
        differs = 0
        for p in range(3):
            for i, (a, e_) in enumerate(runs):
                want = call_twin.logprob(case.twin, a, e_, lab_seg, paths[p], case.constrain)
                wrong = call_twin.logprob(case.twin, a, e_, wrong_lab, paths[p], case.constrain)
                assert abs(np.exp(got[p, i]) - np.exp(want)) <= (e_ - a + 1) * 1e-9, (p, a, e_)
                differs += abs(np.exp(wrong) - np.exp(want)) > 1e-6
        assert differs >= 3
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
    _check_against_twin(case, _paths(case)[0], case.queries(), tag='mixed model')
    # the other way round
    m2 = _fitted(hip, 40, 3, 4, seed=3, transition_model=1)
    assert m2.model.transition_model == 1
    m2.model.transition_model = 0
    case2 = Case(m2)
    assert not np.array_equal(np.array(m2.model.log_transmat), T0)
    _check_against_twin(case2, _paths(case2)[0], case2.queries()[:5], tag='mixed model 1 -> 0')


def test_invariance(hip):
    from remixt_amd.restarts import RestartGroups, RestartSet
    e = synthetic.make_experiment(80, num_clones=3, max_copy_number=4, num_chains=3, seed=4)
    ps = synthetic.make_init_params(e, 4, 4)
    rs = RestartSet(e, ps, 4, num_clones=3, quiet=True, seeds=list(range(4)))
    rs.variational_update(2)
    b, m = rs.batch, rs.models[0]
    _, labels = posteriors.event_tables(b.cn_classes)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    regions = [(i, j) for i in range(0, 70, 7) for j in (i, i + 1, i + 9)]
    runs, _, constrain = posteriors.region_queries(regions, m.seg_fwd_remap, m.seg_is_original, cs, ce)
    post = np.stack([b.get_array(r, 'posterior_marginals') for r in range(4)])
    order = np.argsort(post, axis=2, kind='stable')
    X = order[:, :, -1].astype(np.int16); X[:, ::5] = order[:, ::5, -2]
    paths = np.stack([X] + [np.roll(X, k, axis=1) % b.num_cn_states for k in range(1, 8)], axis=1)      # (4, 8, N1): X in slot 0
    q = np.array([[a, e_, li, 0] for a, e_ in runs for li in (-1, 0, 1, 2)], dtype=np.int32)
    full = b.call_logprob_raw(0, 4, paths, q, labels, constrain)
    assert full.shape == (4, len(q)) and not np.array_equal(full[0], full[1]) and np.isfinite(full).any()
    for r in range(4):
        assert np.array_equal(b.call_logprob_raw(r, 1, paths[r:r + 1], q, labels, constrain)[0], full[r], equal_nan=True)
    assert np.array_equal(b.call_logprob_raw(1, 2, paths[1:3], q, labels, constrain), full[1:3], equal_nan=True)
    for i in range(0, len(q), 5):
        assert np.array_equal(b.call_logprob_raw(0, 4, paths, q[i:i + 1], labels, constrain)[:, 0], full[:, i], equal_nan=True)
    assert np.array_equal(b.call_logprob_raw(0, 4, paths, q[::-1].copy(), labels, constrain), full[:, ::-1], equal_nan=True)
    # one path against eight, the queried path in another slot
    assert np.array_equal(b.call_logprob_raw(0, 4, paths[:, :1], q, labels, constrain), full, equal_nan=True)
    moved = np.ascontiguousarray(paths[:, ::-1]); q7 = q.copy(); q7[:, 3] = 7
    assert np.array_equal(b.call_logprob_raw(0, 4, moved, q7, labels, constrain), full, equal_nan=True)
    # the public forms: the set against one model, and against the groups
    cnX = [b.states_to_cn(X[r])[rs.models[r].seg_fwd_remap] for r in range(4)]
    per_set, lq_set = rs.call_confidence(regions, cnX), rs.cn_logprob(cnX)
    one = rs.models[2].call_confidence(regions, cnX[2])
    for k in posteriors.CALL_ARRAYS:
        assert per_set[k].shape == (4, len(regions)) and np.array_equal(per_set[k][2], one[k]), k
        assert ((per_set[k] >= 0) & (per_set[k] <= 1)).all(), k
    assert lq_set.shape == (4,) and lq_set[2] == rs.models[2].cn_logprob(cnX[2])
    dec_set, dec_lq = rs.call_confidence(regions), rs.cn_logprob()
    assert np.array_equal(dec_set['p_call'][1], rs.models[1].call_confidence(regions)['p_call']) and dec_lq[1] == rs.models[1].cn_logprob()
    assert (dec_lq > lq_set).all()
    rs.close()
    groups = RestartGroups(e, ps, 4, groups=2, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    single = RestartGroups(e, ps, 4, groups=1, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    for g in (groups, single):
        g.variational_update(2)
    for cn in (None, cnX):
        a, c = groups.call_confidence(regions, cn), single.call_confidence(regions, cn)
        for k in posteriors.CALL_ARRAYS:
            assert a[k].shape == (4, len(regions)) and np.array_equal(a[k], c[k]), k
        assert np.array_equal(groups.cn_logprob(cn), single.cn_logprob(cn))
    groups.close(); single.close()


def test_no_side_effects(hip):
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    before = _model_state(m1)
    conf = m1.call_confidence([(0, 10), (5, 5), (20, 49)])
    lq = m1.cn_logprob()
    assert set(conf) == set(posteriors.CALL_ARRAYS) and lq <= 0
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
    _, labels = posteriors.event_tables(b.cn_classes)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    N, S = b.num_segments, b.num_cn_states
    paths = np.zeros((1, 2, N), dtype=np.int16)
    ok = [[int(cs[0]), int(cs[0]) + 1, 0, 0]]
    with pytest.raises(ValueError, match='update_p_cn'):
        b.call_logprob_raw(r, 1, paths, ok, labels)
    assert bpmodel.last_error_restarts() == [r]
    with pytest.raises(ValueError, match='update_p_cn'):
        m.call_confidence([(0, 3)], np.ones((m.N, 3, 2), dtype=int))
    m.variational_update()
    bad = [([[3, 2, -1, 0]], 'first <= last'), ([[-1, 2, -1, 0]], 'first <= last'), ([[0, N, -1, 0]], 'first <= last'),
           ([[int(ce[0]), int(ce[0]) + 1, -1, 0]], 'chain end'), ([[int(cs[0]), int(ce[1]), -1, 0]], 'chain end'),
           ([[0, 1, len(LABELS), 0]], 'label index'), ([[0, 1, -2, 0]], 'label index'), ([[0, 1, -1, 2]], 'path index'),
           ([[0, 1, -1, -1]], 'path index')]
    for q, text in bad:
        with pytest.raises(ValueError, match='^bad argument: .*' + text):
            b.call_logprob_raw(r, 1, paths, ok + q, labels)
        assert bpmodel.last_error_restarts() == []
    with pytest.raises(ValueError, match='^bad argument: .*label index'):      # an index without a table
        b.call_logprob_raw(r, 1, paths, ok, None)
    for entry in (-1, S):
        p2 = paths.copy(); p2[0, 1, N - 1] = entry                       # (in a path no query reads)
        with pytest.raises(ValueError, match='^bad argument: .*path entry'):
            b.call_logprob_raw(r, 1, p2, ok, labels)
    for args in ((r + 1, 1), (-1, 1)):
        with pytest.raises(ValueError, match='^bad argument: bad restart range$'):
            b.call_logprob_raw(args[0], args[1], paths, ok, labels)
    for kw in (dict(queries=[[0, 1, 0]]), dict(paths=paths[:, :, :-1]), dict(paths=paths[0]), dict(labels=labels[:1, :, :-1]), dict(constrain=np.ones(N + 1))):
        args = dict(paths=paths, queries=ok, labels=labels, constrain=None); args.update(kw)
        with pytest.raises(ValueError, match='must have shape'):
            b.call_logprob_raw(r, 1, **args)
    # the C entry point itself: RMX_EARG leaves the output untouched
    i16p, i32p, u8p, dp = C.POINTER(C.c_int16), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    lab = np.ascontiguousarray(labels, dtype=np.int16)

    def call(r0, nr, npaths, pt, queries):
        q = np.ascontiguousarray(ok if queries is None else queries, dtype=np.int32).reshape(-1, 4)
        out = np.full(max(len(q), 1), 12345.)
        nq = -1 if queries is None else len(q)      # (None: a negative count)
        rc = b._lib.rmx_call_prob(b._handle, r0, nr, npaths, pt.ctypes.data_as(i16p), nq, q.ctypes.data_as(i32p) if len(q) else i32p(),
                                  lab.shape[1], lab.ctypes.data_as(i16p), u8p(), out.ctypes.data_as(dp))
        return rc, out
    pt = np.ascontiguousarray(paths)
    for q, _ in bad:
        rc, out = call(r, 1, 2, pt, ok + q)
        assert rc == bpmodel.RMX_EARG and (out == 12345.).all()
    p2 = pt.copy(); p2[0, 0, 3] = S
    for args in ((r, 1, 2, p2, ok), (r, 1, 0, pt, ok), (r, 0, 2, pt, ok), (r + 1, 1, 2, pt, ok), (r, 1, 2, pt, None)):
        rc, out = call(*args)
        assert rc == bpmodel.RMX_EARG and (out == 12345.).all(), args[:3]
    rc, out = call(r, 1, 2, pt, np.zeros((0, 4)))                         # no queries: valid, nothing to do
    assert rc == 0 and (out == 12345.).all()
    rc, out = call(r, 1, 2, pt, ok)
    assert rc == 0 and out[0] <= 0
    assert b.call_logprob_raw(r, 1, paths, ok, labels).shape == (1, 1)
    assert b.call_logprob_raw(r, 1, paths, np.zeros((0, 4), dtype=np.int32), labels).shape == (1, 0)
    with pytest.raises(ValueError):
        m.call_confidence([(4, 2)])
    with pytest.raises(ValueError, match='not in its segment'):
        m.cn_logprob(np.full((m.N, 3, 2), 9))


def test_pipeline_cn_call_confidence(hip, tmp_path):
    from remixt_amd import workflow
    from remixt_amd.analysis import pipeline
    from remixt_amd.restarts import RestartSet
    import pickle
    e, config, init_params = _pipeline_case()
    ids = sorted(init_params)
    seeds = [100 + i for i in ids]
    cn_regions = [('geneA', 10, 14), ('arm', 0, 250), ('seg', 77, 77), ('pair', 300, 301)]
    base = pipeline.fit_restarts(e, init_params, config, seeds=seeds, groups=1)
    off = pipeline.fit_restarts(e, init_params, dict(config, cn_call_confidence=False), seeds=seeds, groups=1)
    on = pipeline.fit_restarts(e, init_params, dict(config, cn_regions=cn_regions, cn_call_confidence=True), seeds=seeds, groups=1)
    # off: the results of a run that never heard of it; on: the same results plus region_events (cn_regions), call_confidence and the stat
    assert not any('call_confidence' in res or 'cn_logprob' in res['stats'] for res in base.values())
    _same_results(base, off)
    _same_results(base, dict((i, dict(((k, v) if k != 'stats' else (k, dict((sk, sv) for sk, sv in v.items() if sk != 'cn_logprob')))
                                      for k, v in res.items() if k not in ('call_confidence', 'region_events'))) for i, res in on.items()))
    assert all('region_events' in res for res in on.values())
    # recomputation from the same fit
    rs = RestartSet(e, [init_params[i] for i in ids], 4, num_clones=3, quiet=True, seeds=seeds, **pipeline._model_kwargs(e, config))
    rs.fit(config['num_em_iter'], config['num_update_iter'])
    cn = [on[i]['cn'] for i in ids]
    want, want_lq = rs.call_confidence([(a, b) for _, a, b in cn_regions], cn), rs.cn_logprob(cn)
    assert np.array_equal(want_lq, rs.cn_logprob())                      # (the result's cn is the decoded path)
    rs.close()
    for j, i in enumerate(ids):
        cc = on[i]['call_confidence']
        assert cc['names'] == ['geneA', 'arm', 'seg', 'pair'] and sorted(cc) == sorted(posteriors.CALL_ARRAYS + ('names',))
        for k in posteriors.CALL_ARRAYS:
            assert cc[k].shape == (4,) and ((cc[k] >= 0) & (cc[k] <= 1)).all() and np.array_equal(cc[k], want[k][j]), (i, k)
        assert (cc['p_call'] <= cc['p_call_unphased'] + 1e-12).all() and (cc['p_call_unphased'] <= cc['p_call_total'] + 1e-12).all()
        assert on[i]['stats']['cn_logprob'] == want_lq[j] and want_lq[j] <= 0
    one = pipeline.fit(e, init_params[ids[1]], dict(config, cn_regions=cn_regions, cn_call_confidence=True), quiet=True, init_id=ids[1])
    assert one['call_confidence']['names'] == on[ids[1]]['call_confidence']['names'] and one['call_confidence']['p_call'].shape == (4,)
    assert np.isfinite(one['stats']['cn_logprob'])
    # the workflow (fit_restarts_distributed + collate): the arrays in the record and in the store
    exp_file = str(tmp_path / 'experiment.pickle')
    with open(exp_file, 'wb') as f:
        pickle.dump(e, f)
    workflow.fit_model(exp_file, str(tmp_path / 'r.store'), dict(config, cn_regions=cn_regions, cn_call_confidence=True), None)
    with pipeline._Store(str(tmp_path / 'r.store'), 'r') as st:
        assert 'cn_logprob' in st['stats'].columns and (st['stats']['cn_logprob'] <= 0).all()
        for i in sorted(st['stats']['init_id']):
            for k in posteriors.CALL_ARRAYS:
                v = np.asarray(st['solutions/solution_%d/%s' % (i, k)])
                assert v.shape == (4,) and ((v >= 0) & (v <= 1)).all(), (i, k)
    workflow.fit_model(exp_file, str(tmp_path / 'r0.store'), dict(config, cn_regions=cn_regions), None)
    with pipeline._Store(str(tmp_path / 'r0.store'), 'r') as st:
        assert not any('p_call' in k for k in st.keys()) and 'cn_logprob' not in st['stats'].columns


def test_full_size(hip):
    """50 000 segments, 165 states, 16 restarts: every three-segment window under three labels and the 23 whole chains,
    for the decoded paths, in one call (timed, no time asserted)."""
    from remixt_amd.restarts import RestartSet
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=8, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, 16, 8)
    rs = RestartSet(e, ps, 8, num_clones=3, quiet=True, seeds=list(range(16)))
    try:
        rs.variational_update(1)
        b, m = rs.batch, rs.models[0]
        S, N1 = b.num_cn_states, b.num_segments
        assert S == 165
        _, labels = posteriors.event_tables(b.cn_classes)
        cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
        states = rs._call_states(None)
        assert states.shape == (16, N1)
        chain = np.searchsorted(ce, np.arange(N1), side='left')
        a = np.flatnonzero(chain[:-2] == chain[2:]) if N1 > 2 else np.zeros(0, dtype=int)
        win = np.stack([a, a + 2], axis=1)
        q = np.concatenate([np.concatenate([win, np.full((len(win), 1), LABELS.index(lb)), np.zeros((len(win), 1), dtype=int)], axis=1)
                            for _, lb in posteriors.CALL_LABELS]
                           + [np.stack([cs, ce, np.full(len(cs), -1), np.zeros(len(cs), dtype=int)], axis=1)]).astype(np.int32)
        pick = np.random.RandomState(0).choice(N1, size=1000, replace=False)
        q = np.concatenate([q, np.stack([pick, pick, np.full(1000, -1), np.zeros(1000, dtype=int)], axis=1).astype(np.int32)])
        constrain = np.asarray(m.seg_is_original, dtype=bool)
        b.call_logprob_raw(0, 16, states[:, None], q[:64], labels, constrain)
        b.profile_reset(); b.profile_enable(1)
        t0 = time.perf_counter()
        lp = b.call_logprob_raw(0, 16, states[:, None], q, labels, constrain)
        wall = time.perf_counter() - t0
        ms, launches = b.profile()['k_call_prob']; b.profile_enable(0)
        print('call_logprob_raw, 16 restarts x %d queries (%d windows x 3 labels, %d chains, 1000 segments): %.1f ms wall, k_call_prob %.2f ms device in %d launches' % (
            len(q), len(win), len(cs), wall * 1e3, ms, launches))
        assert lp.shape == (16, len(q)) and launches == 1 and not np.isnan(lp).any() and (lp <= 3 * (4 * S + 32) * U * N1).all()
        W = len(win)
        assert (lp[:, :W] <= lp[:, W:2 * W] + 3 * (4 * S + 32) * U).all() and (lp[:, W:2 * W] <= lp[:, 2 * W:3 * W] + 3 * (4 * S + 32) * U).all()
        # identity (a) at the 1 000 segments, restart 1
        post = b.get_array(1, 'posterior_marginals')
        got = lp[1, -1000:]
        want = np.where(constrain[pick], post[pick, states[1, pick]], 1.)
        assert np.array_equal(got == -np.inf, want == 0)
        ok = want > 0
        tol = ((S + 4) + 3 * np.abs(np.log(want[ok]))) * U
        bound = constrain[pick][ok]
        assert (np.abs(np.exp(got[ok]) / want[ok] - 1)[bound] <= tol[bound]).all() and (np.abs(got[ok][~bound]) <= (S + 4) * U).all()
        del post
    finally:
        rs.close()
