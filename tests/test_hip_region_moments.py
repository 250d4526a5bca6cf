"""Region moments on the device (rmx_region_moments / k_region_moments): against the numpy twin on the read-back
framelogprob / log_transmat, the identities that tie them to the marginals and to rmx_region_prob, the sampler, two state
classes, the mixed transition model, inserted segments, invariance to batching and grouping, no side effects on the
model, errors, the pipeline, and a chunked launch."""
import ctypes as C

import numpy as np
import pytest

from remixt_amd import posteriors, synthetic
from tests import helpers as H
from tests import region_moments_twin
from tests.test_hip_region_events import MASKS, Case
from tests.test_hip_sample_cn import GRIDS, _fitted, _model_state, _pipeline_case, _same_results

pytestmark = pytest.mark.gpu

U = 2. ** -53
W_LEN, W_ONE, W_LEN2, W_ONE2 = 0, 1, 2, 3      # rows of a case's weight table: lengths, ones, and both doubled


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


class MomentsCase(Case):
    """Case with the feature table of posteriors.moment_features plus one random real-valued feature, the weight table
    (lengths, ones, 2 lengths, twos) and the moments twin."""

    def __init__(self, m, l1=None, **kw):
        Case.__init__(self, m, **kw)
        self.mtwin = region_moments_twin.MomentsTwin(self.twin)
        b = self.b
        F = posteriors.moment_features(b.cn_classes)
        self.M = F.shape[1] - 4
        rnd = np.random.RandomState(5).normal(size=(F.shape[0], 1, self.S))
        self.feats = np.ascontiguousarray(np.concatenate([F, rnd], axis=1))           # (C, M + 5, S)
        self.feat_seg = self.feats[b.seg_class]                                       # (N, M + 5, S)
        l1 = np.asarray(m.l1 if l1 is None else l1, dtype=float)
        self.weights = np.stack([l1, np.ones(self.N), 2 * l1, 2 * np.ones(self.N)])
        # (first feature, number of features): the totals, the fractions, the random feature alone
        self.groups = [(0, self.M), (self.M, 4), (self.M + 4, 1)]

    def moments(self, runs, f0, nf, wi, r0=None, nr=1):
        q = np.array([[a, e, f0, wi] for a, e in runs], dtype=np.int32)
        return self.b.region_moments_raw(self.r if r0 is None else r0, nr, q, self.feats, self.weights, nf)

    def bound(self, a, e, f0, nf, wi):
        """B_f = sum_n |w_n| max_s |phi_f(s)| over the run."""
        seg = np.arange(a, e + 1)
        return (np.abs(self.weights[wi, seg])[:, None] * np.abs(self.feat_seg[seg, f0:f0 + nf]).max(axis=2)).sum(axis=0)

    def check_against_twin(self, runs, groups=None, weights=(W_LEN, W_ONE), tag=''):
        worst_m = worst_c = 0.
        for f0, nf in (self.groups if groups is None else groups):
            for wi in weights:
                got = self.moments(runs, f0, nf, wi)[0]
                assert got.shape == (len(runs), nf + nf * (nf + 1) // 2)
                gm, gc = posteriors._moment_matrices(got, nf)
                for i, (a, e) in enumerate(runs):
                    L = e - a + 1
                    B = self.bound(a, e, f0, nf, wi)
                    wm, wc = self.mtwin.moments(a, e, self.feat_seg[:, f0:f0 + nf], self.weights[wi])
                    em, ec = np.abs(gm[i] - wm), np.abs(gc[i] - wc)
                    BB = np.outer(B, B)
                    rm = (em[B > 0] / B[B > 0]).max() if (B > 0).any() else 0.
                    rc = (ec[BB > 0] / BB[BB > 0]).max() if (BB > 0).any() else 0.
                    worst_m, worst_c = max(worst_m, rm / L), max(worst_c, rc / L)
                    print('%s run [%d, %d] features %d..%d weights %d: |mean - twin| / B %.3e, |cov - twin| / B^2 %.3e' % (tag, a, e, f0, f0 + nf - 1, wi, rm, rc))
                    assert (em <= L * 1e-9 * B).all(), (tag, a, e, f0, nf, wi, gm[i], wm)
                    assert (ec <= L * 1e-9 * BB).all(), (tag, a, e, f0, nf, wi, gc[i], wc)
        print('%s worst |mean - twin| / (L B): %.3e, worst |cov - twin| / (L B^2): %.3e' % (tag, worst_m, worst_c))


@pytest.fixture(scope='module')
def cases(hip):
    return dict(((N, M, c), MomentsCase(_fitted(hip, N, M, c))) for N, M, c in GRIDS)


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_twin(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    assert case.S == {8: 165, 12: 355, 6: 457}[max_cn] and case.S % 64 and case.S % 16 and case.M == M
    assert case.m.num_breakpoints > 0 and (case.bidx >= 0).any()
    b = case.b
    b.profile_reset(); b.profile_enable(1)
    case.moments(case.queries(), case.M, 4, W_LEN)
    prof = b.profile(); b.profile_enable(0)
    assert prof['k_region_moments'][1] == 1 and prof['k_region_moments'][0] > 0      # one launch for one call
    case.check_against_twin(case.queries(), tag='S %d' % case.S)
    # the model-level form
    q = np.array([[a, e, 0, W_ONE] for a, e in case.queries()], dtype=np.int32)
    one = case.m.model.region_moments(q, case.feats, case.weights, 2)
    assert one.shape == (len(q), 5) and np.array_equal(one, b.region_moments_raw(case.r, 1, q, case.feats, case.weights, 2)[0])


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_identities(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    b, S, Mc = case.b, case.S, case.M
    post = b.get_array(case.r, 'posterior_marginals').astype(np.longdouble)
    # (1) a one-segment run is the segment's own covariance under its marginal
    single = [(n, n) for n in range(case.N)]
    worst = 0.
    for f0, nf in case.groups:
        for wi in (W_LEN, W_ONE):
            gm, gc = posteriors._moment_matrices(case.moments(single, f0, nf, wi)[0], nf)
            for n in range(case.N):
                phi, w = case.feat_seg[n, f0:f0 + nf].astype(np.longdouble), case.weights[wi, n]
                E1 = (post[n] * phi).sum(axis=1)
                E2 = (post[n] * phi[:, None, :] * phi[None, :, :]).sum(axis=2)
                want = (w * w * (E2 - np.outer(E1, E1))).astype(float)
                B = case.bound(n, n, f0, nf, wi)
                err = np.abs(gc[n] - want)
                BB = np.outer(B, B)
                if (BB > 0).any():
                    worst = max(worst, (err[BB > 0] / BB[BB > 0]).max())
                assert (err <= (4 * S + 32) * U * BB).all(), (n, f0, nf, wi, gc[n], want)
    print('S %d one segment: worst |cov - marginal covariance| / B^2 %.3e (bound %.3e)' % (S, worst, (4 * S + 32) * U))
    # (2) an indicator with unit weights: the mean is the sum of the marginal probabilities, and the variance of an adjacent
    # pair comes from the joint probability of rmx_region_prob (constrain NULL: the mask binds inserted segments too)
    # (with a normal clone of (1, 1) no state of these grids is LOH, so `loh` checks the zeros; `subclonal` has mass)
    c = int(np.argmax(case.ce - case.cs))
    seg = np.arange(case.cs[c], case.ce[c] + 1)
    runs = [(int(a), int(e)) for a in seg for e in seg if a <= e]
    pairs = [(int(a), int(a) + 1) for a in seg[:-1]]
    for name in ('loh', 'subclonal'):
        ind = Mc + posteriors.MOMENT_FRACTIONS.index(name)
        p = (post * case.mask_seg[name]).sum(axis=1).astype(float)
        got = case.moments(runs, ind, 1, W_ONE)[0]
        for (a, e), row in zip(runs, got):
            assert abs(row[0] - p[a:e + 1].sum()) <= (e - a + 1) * 1e-9, (name, a, e, row[0])
        if pairs:
            q = np.array([[a, e, MASKS.index(name), -1] for a, e in pairs], dtype=np.int32)
            both = np.exp(b.region_logprob_raw(case.r, 1, q, case.masks, None, None)[0])
            var = case.moments(pairs, ind, 1, W_ONE)[0][:, 1]
            want = np.array([p[a] * (1 - p[a]) + p[e] * (1 - p[e]) + 2 * (pb - p[a] * p[e]) for (a, e), pb in zip(pairs, both)])
            print('S %d adjacent pairs, %s: max |Var - identity| %.3e, max Var %.3e' % (S, name, np.abs(var - want).max(), var.max()))
            assert (np.abs(var - want) <= 2e-9).all(), (name, var, want)
    # (3) the covariance matrix of a group is symmetric (one number per pair) and positive semi-definite up to the budget
    for f0, nf in case.groups[:2]:
        for wi in (W_LEN, W_ONE):
            _, gc = posteriors._moment_matrices(case.moments(runs, f0, nf, wi)[0], nf)
            for (a, e), cv in zip(runs, gc):
                assert np.array_equal(cv, cv.T)
                B = case.bound(a, e, f0, nf, wi)
                assert np.linalg.eigvalsh(cv).min() >= -(e - a + 1) * 1e-9 * (B.max() ** 2), (a, e, f0, wi, np.linalg.eigvalsh(cv))
    # (4) doubling the weights doubles the means and quadruples the covariances, exactly
    some = case.queries()
    for f0, nf in case.groups:
        for w1, w2 in ((W_LEN, W_LEN2), (W_ONE, W_ONE2)):
            x1, x2 = case.moments(some, f0, nf, w1)[0], case.moments(some, f0, nf, w2)[0]
            assert np.array_equal(x2[:, :nf], 2 * x1[:, :nf]) and np.array_equal(x2[:, nf:], 4 * x1[:, nf:]), (f0, nf, w1)
    # (5) a feature's mean and variance do not depend on the other features of its query: the compaction of a step does not look
    # at the columns, so nf = 1 queries reproduce the nf = 4 query's entries bit for bit
    four = case.moments(some, Mc, 4, W_LEN)[0]
    diag = 4 + np.array([0, 4, 7, 9])                # (f, f) of the upper triangle of a 4 x 4 matrix, after the 4 means
    for k in range(4):
        one = case.moments(some, Mc + k, 1, W_LEN)[0]
        assert np.array_equal(one[:, 0], four[:, k]) and np.array_equal(one[:, 1], four[:, diag[k]]), k


def test_against_the_sampler(hip):
    """The masked case of test_hip_region_counts.test_against_the_sampler (experiment seed 0), 4 096 samples of seed 99: the
    sample mean and variance of every F_f of every run of Case.queries() against the exact ones.  The twin over the oracle
    kernel module's arrays of this case gives, among these runs, the eight features and the two weight vectors, 70 of
    112 (run, feature, weights) triples whose exact SD is above 1 % of the run's B_f: with the read counts masked the
    posterior is spread over many states at every segment."""
    from tests.test_hip_posterior_summary import _fitted as fitted_masked
    m = fitted_masked(hip, 30, 3, 8, sweeps=3, masked=True)
    case = MomentsCase(m)
    NS = 4096
    st = case.b.sample_states(case.r, 1, NS, [99]).astype(np.int64)[0]
    runs = case.queries()
    informative = 0
    for f0, nf in case.groups:
        for wi in (W_LEN, W_ONE):
            gm, gc = posteriors._moment_matrices(case.moments(runs, f0, nf, wi)[0], nf)
            for i, (a, e) in enumerate(runs):
                B = case.bound(a, e, f0, nf, wi)
                for k in range(nf):
                    F = np.zeros(NS)
                    for n in range(a, e + 1):
                        F += case.weights[wi, n] * case.feat_seg[n, f0 + k, st[:, n]]
                    mean, var = gm[i, k], max(gc[i, k, k], 0.)
                    d = F - F.mean()
                    svar, m4 = (d ** 2).mean(), (d ** 4).mean()
                    informative += np.sqrt(var) > 0.01 * B[k]
                    assert abs(F.mean() - mean) <= 6 * np.sqrt(var / NS) + 1e-9 * B[k], (a, e, f0 + k, wi, F.mean(), mean)
                    assert abs(svar - var) <= 6 * np.sqrt(max(m4 - var * var, 0.) / NS) + B[k] ** 2 / NS, (a, e, f0 + k, wi, svar, var)
    print('informative (run, feature, weights) triples: %d' % informative)
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
        case = MomentsCase(m, batch=b, r=0)
        loh = M + posteriors.MOMENT_FRACTIONS.index('loh')
        assert not case.feats[0, loh].any() and case.feats[1, loh].any()          # the LOH indicator differs per class
        assert (case.feats[0, 0] == 2).all() and (case.feats[1, 0] == 1).all()    # and so does the normal clone's total
        case.check_against_twin(case.queries(), tag='two classes')
        # (a kernel that took class 0's table everywhere would see no LOH and a normal total of 2 at every segment)
        odd, even = [(n, n) for n in range(1, N, 2)], [(n, n) for n in range(0, N, 2)]
        assert (case.moments(even, loh, 1, W_ONE)[0] == 0).all() and (case.moments(odd, loh, 1, W_ONE)[0][:, 0] > 0).any()
        assert np.array_equal(case.moments(odd, 0, 1, W_ONE)[0][:, 0], np.ones(len(odd)))
        assert np.array_equal(case.moments(even, 0, 1, W_ONE)[0][:, 0], 2 * np.ones(len(even)))
    finally:
        b.close()


def test_mixed_transition_model(hip):
    """The snapshot of the last update_p_cn under another transition_model than the current one, both directions."""
    m = _fitted(hip, 40, 3, 4, seed=3)
    T0 = np.array(m.model.log_transmat)
    m.model.transition_model = 1
    assert np.array_equal(np.array(m.model.log_transmat), T0)            # the snapshot stays the model-0 one
    case = MomentsCase(m)
    case.check_against_twin(case.queries(), tag='mixed model')
    m2 = _fitted(hip, 40, 3, 4, seed=3, transition_model=1)
    assert m2.model.transition_model == 1
    m2.model.transition_model = 0
    case2 = MomentsCase(m2)
    assert not np.array_equal(np.array(m2.model.log_transmat), T0)
    case2.check_against_twin(case2.queries(), tag='mixed model 1 -> 0')


def test_inserted_segments(hip):
    """Two breakends on one boundary: the model inserts a zero-length segment there.  Length weights ignore it; with unit
    weights it counts like any other segment."""
    e = synthetic.make_experiment(60, num_clones=3, max_copy_number=4, num_chains=3, seed=7)
    e.breakpoints = H.add_shared_boundary_breakpoints(e)
    m, h, _ = H.make_model(hip, M=3, max_cn=4, experiment=e)
    H.attach(m, h)
    m.variational_update(); m.variational_update()
    case = MomentsCase(m)
    assert m.N1 > m.N and not case.constrain.all()
    dummy = int(np.flatnonzero(~case.constrain & (np.arange(m.N1) > 0) & (case.tel == 0))[0])
    assert case.constrain[dummy - 1] and case.constrain[dummy + 1] and case.weights[W_LEN, dummy] == 0
    runs = [(dummy - 1, dummy + 1), (dummy, dummy), (dummy, dummy + 1)]
    case.check_against_twin(runs, tag='inserted segment')
    # the inserted segment alone: nothing under length weights, its own moments under unit weights
    assert (case.moments([(dummy, dummy)], 0, 3, W_LEN)[0] == 0).all()
    unit = case.moments([(dummy, dummy)], 0, 3, W_ONE)[0, 0]
    assert (unit[:3] > 0).all() and unit[3 + 3] > 0      # (a tumour clone's total varies there)
    # the experiment pair around it, through region_cn_moments
    i = int(m.seg_rev_remap[dummy - 1])
    assert m.seg_fwd_remap[i] == dummy - 1 and m.seg_fwd_remap[i + 1] == dummy + 1
    out = m.region_cn_moments([(i, i + 1), (i, i)])
    assert sorted(out) == sorted(posteriors.MOMENT_ARRAYS)
    l1 = case.weights[W_LEN]
    L = l1[dummy - 1] + l1[dummy + 1]
    assert abs(out['length'][0] - L) <= 1e-9 * L and abs(out['length'][1] - l1[dummy - 1]) <= 1e-9 * L
    for name, sl in (('total_cn', slice(0, 3)), ('fraction', slice(3, 7))):
        wm, wc = case.mtwin.moments(dummy - 1, dummy + 1, case.feat_seg[:, sl], l1)
        top = np.abs(case.feat_seg[:, sl]).max(axis=(0, 2))
        assert out[name + '_mean'].shape == (2, len(top)) and out[name + '_cov'].shape == (2, len(top), len(top))
        assert (np.abs(out[name + '_mean'][0] - wm / L) <= 3e-9 * top).all(), name
        assert (np.abs(out[name + '_cov'][0] - wc / L ** 2) <= 3e-9 * np.outer(top, top)).all(), name
    sd = m.ploidy_posterior_sd()
    assert np.isfinite(sd) and sd >= 0


def test_invariance(hip):
    from remixt_amd.restarts import RestartGroups, RestartSet
    e = synthetic.make_experiment(80, num_clones=3, max_copy_number=4, num_chains=3, seed=4)
    ps = synthetic.make_init_params(e, 4, 4)
    rs = RestartSet(e, ps, 4, num_clones=3, quiet=True, seeds=list(range(4)))
    rs.variational_update(2)
    b, m = rs.batch, rs.models[0]
    feats = posteriors.moment_features(b.cn_classes)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    regions = [(i, j) for i in range(0, 70, 7) for j in (i, i + 1, i + 9)]
    runs, _, _ = posteriors.region_queries(regions, m.seg_fwd_remap, m.seg_is_original, cs, ce)
    weights = np.stack([np.asarray(m.l1, dtype=float), np.ones(b.num_segments)])
    q = np.array([[a, e_, f0, wi] for a, e_ in runs for f0, wi in ((0, 0), (3, 1), (4, 0))], dtype=np.int32)
    call = lambda r0, nr, qq: b.region_moments_raw(r0, nr, qq, feats, weights, 3)
    full = call(0, 4, q)
    assert full.shape == (4, len(q), 9) and not np.array_equal(full[0], full[1]) and np.isfinite(full).all()
    for r in range(4):
        assert np.array_equal(call(r, 1, q)[0], full[r])
    assert np.array_equal(call(1, 2, q), full[1:3])
    for i in range(0, len(q), 5):
        assert np.array_equal(call(0, 4, q[i:i + 1])[:, 0], full[:, i])
    assert np.array_equal(call(0, 4, q[::-1].copy()), full[:, ::-1])
    per_set = rs.region_cn_moments(regions)
    one = rs.models[2].region_cn_moments(regions)
    shapes = posteriors.moment_shapes(len(regions), 3)
    assert np.array_equal(per_set['length'], one['length']) and per_set['length'].shape == shapes['length']
    for k in posteriors.MOMENT_ARRAYS[1:]:
        assert per_set[k].shape == (4,) + shapes[k] and np.array_equal(per_set[k][2], one[k]), k
    rs.close()
    groups = RestartGroups(e, ps, 4, groups=2, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    single = RestartGroups(e, ps, 4, groups=1, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    for g in (groups, single):
        g.variational_update(2)
    a, c = groups.region_cn_moments(regions), single.region_cn_moments(regions)
    for k in posteriors.MOMENT_ARRAYS:
        assert np.array_equal(a[k], c[k]), k
    assert a['total_cn_cov'].shape == (4,) + shapes['total_cn_cov']
    groups.close(); single.close()


def test_no_side_effects(hip):
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    before = _model_state(m1)
    out = m1.region_cn_moments([(0, 10), (5, 5), (20, 49)])
    assert set(out) == set(posteriors.MOMENT_ARRAYS) and out['total_cn_cov'].shape == (3, 3, 3)
    m1.ploidy_posterior_sd()
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


def _c_call(b, r, q, feats, weights, nf, out, null=None):
    """rmx_region_moments through ctypes with the caller's output buffer: the return code."""
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    q = np.ascontiguousarray(q, dtype=np.int32).reshape(-1, 4)
    feats, weights = np.ascontiguousarray(feats, dtype=np.float64), np.ascontiguousarray(weights, dtype=np.float64)
    return b._lib.rmx_region_moments(b._handle, r, 1, len(q), q.ctypes.data_as(ip) if len(q) else ip(), feats.shape[1],
                                     dp() if null == 'features' else feats.ctypes.data_as(dp), weights.shape[0],
                                     dp() if null == 'weights' else weights.ctypes.data_as(dp), nf, out.ctypes.data_as(dp))


def test_errors(hip):
    from remixt_amd import bpmodel
    m, h, e = H.make_model(hip, N=30, M=3, max_cn=3)
    H.attach(m, h)
    b, r = m.model._batch, m.model._r
    feats = posteriors.moment_features(b.cn_classes)
    N = b.num_segments
    weights = np.stack([np.asarray(m.l1, dtype=float), np.ones(N)])
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    ok = [[int(cs[0]), int(cs[0]) + 1, 0, 0]]
    out = np.full(64, -7.)
    # before update_p_cn: RMX_EVALUE with the restart listed
    assert _c_call(b, r, ok, feats, weights, 3, out) == bpmodel.RMX_EVALUE and (out == -7.).all()
    with pytest.raises(ValueError, match='update_p_cn'):
        b.region_moments_raw(r, 1, ok, feats, weights, 3)
    assert bpmodel.last_error_restarts() == [r]
    with pytest.raises(ValueError, match='update_p_cn'):
        m.region_cn_moments([(0, 3)])
    m.variational_update()
    b.profile_reset(); b.profile_enable(1)
    assert b.region_moments_raw(r, 1, ok, feats, weights, 3).shape == (1, 1, 9)
    launches = b.profile()['k_region_moments'][1]
    assert launches == 1
    nfeat = feats.shape[1]
    bad_f, bad_w = feats.copy(), weights.copy()
    bad_f[0, 2, 5] = np.nan; bad_w[1, 3] = np.inf
    bad = [(ok, feats, weights, 0, None, r'\[1, 4\]'), (ok, feats, weights, 5, None, r'\[1, 4\]'), (ok, feats[:, :2], weights, 3, None, 'tables'),
           ([], feats, weights, 3, None, 'no queries'), (ok, feats, weights, 3, 'features', 'tables'), (ok, feats, weights, 3, 'weights', 'tables'),
           (ok, bad_f, weights, 3, None, 'feature is not finite'), (ok, feats, bad_w, 3, None, 'weight is not finite'),
           (ok + [[0, 1, nfeat - 2, 0]], feats, weights, 3, None, 'first feature'), (ok + [[0, 1, -1, 0]], feats, weights, 3, None, 'first feature'),
           (ok + [[0, 1, 0, 2]], feats, weights, 3, None, 'weight vector index'), (ok + [[0, 1, 0, -1]], feats, weights, 3, None, 'weight vector index'),
           (ok + [[3, 2, 0, 0]], feats, weights, 3, None, 'first <= last'), (ok + [[0, N, 0, 0]], feats, weights, 3, None, 'first <= last'),
           (ok + [[int(ce[0]), int(ce[0]) + 1, 0, 0]], feats, weights, 3, None, 'chain end'), (ok + [[int(cs[0]), int(ce[1]), 0, 0]], feats, weights, 3, None, 'chain end')]
    import re
    for q, ft, wt, nf, null, text in bad:
        assert _c_call(b, r, q, ft, wt, nf, out, null) == bpmodel.RMX_EARG, (q, nf, null, text)
        assert (out == -7.).all(), (q, nf, null, text)                    # the output buffer is untouched
        assert re.search(text, hip._lib.load().rmx_last_error().decode()), (text, hip._lib.load().rmx_last_error())
        assert bpmodel.last_error_restarts() == []
        assert b.profile()['k_region_moments'][1] == launches, (q, nf)     # nothing was launched
    with pytest.raises(ValueError, match='^bad argument: .*first feature'):
        b.region_moments_raw(r, 1, ok + [[0, 1, nfeat, 0]], feats, weights, 1)
    b.profile_enable(0)
    with pytest.raises(ValueError):
        m.region_cn_moments([(4, 2)])


def test_pipeline_region_moments(hip, tmp_path):
    from remixt_amd import restarts, workflow
    from remixt_amd.analysis import pipeline
    import pickle
    e, config, init_params = _pipeline_case()
    ids = sorted(init_params)
    seeds = [100 + i for i in ids]
    cn_regions = [('geneA', 10, 14), ('arm', 0, 250), ('seg', 77, 77), ('pair', 300, 301)]
    R, M = len(cn_regions), 3
    base = pipeline.fit_restarts(e, init_params, dict(config, cn_regions=cn_regions), seeds=seeds, groups=2)
    off = pipeline.fit_restarts(e, init_params, dict(config, cn_regions=cn_regions, cn_region_moments=False), seeds=seeds, groups=2)
    on = pipeline.fit_restarts(e, init_params, dict(config, cn_regions=cn_regions, cn_region_moments=True), seeds=seeds, groups=2)
    strip = lambda results: dict((i, dict((k, (dict((sk, sv) for sk, sv in v.items() if sk not in posteriors.MOMENT_STATS) if k == 'stats' else v))
                                          for k, v in res.items() if k not in ('region_events', 'region_cn_moments'))) for i, res in results.items())
    assert not any('region_cn_moments' in res or any(k in res['stats'] for k in posteriors.MOMENT_STATS) for res in base.values())
    _same_results(strip(base), dict((i, dict((k, v) for k, v in res.items() if k != 'region_events')) for i, res in off.items()))
    _same_results(strip(base), strip(on))
    for i in base:
        for k in posteriors.REGION_ARRAYS:
            assert np.array_equal(base[i]['region_events'][k], on[i]['region_events'][k]) and np.array_equal(base[i]['region_events'][k], off[i]['region_events'][k])
    shapes = posteriors.moment_shapes(R, M)
    for i in ids:
        mom = on[i]['region_cn_moments']
        assert mom['names'] == ['geneA', 'arm', 'seg', 'pair'] and sorted(mom) == sorted(('names',) + posteriors.MOMENT_ARRAYS)
        for k in posteriors.MOMENT_ARRAYS:
            assert mom[k].shape == shapes[k] and np.isfinite(mom[k]).all(), (i, k)
        assert (mom['length'] > 0).all()
        assert (np.diagonal(mom['total_cn_cov'], axis1=1, axis2=2) >= 0).all() and (np.diagonal(mom['fraction_cov'], axis1=1, axis2=2) >= 0).all()
        assert ((mom['fraction_mean'][:, 1:] >= 0) & (mom['fraction_mean'][:, 1:] <= 1 + 1e-12)).all()
        for k in posteriors.MOMENT_STATS:
            assert np.isfinite(on[i]['stats'][k]) and on[i]['stats'][k] >= 0, (i, k)
    one = pipeline.fit(e, init_params[ids[1]], dict(config, cn_regions=cn_regions, cn_region_moments=True), quiet=True, init_id=ids[1])
    assert one['region_cn_moments']['names'] == mom['names'] and one['region_cn_moments']['total_cn_cov'].shape == (R, M, M)
    assert all(np.isfinite(one['stats'][k]) and one['stats'][k] >= 0 for k in posteriors.MOMENT_STATS)
    # the distributed form: the arrays and the stats through the record
    dist = restarts.fit_restarts_distributed(e, [init_params[i] for i in ids], 4, num_clones=3, num_em_iter=config['num_em_iter'],
                                             num_update_iter=config['num_update_iter'], seeds=seeds, quiet=True, cn_regions=cn_regions,
                                             cn_region_moments=True, **pipeline._model_kwargs(e, config))
    for j, i in enumerate(ids):
        assert dist[j]['region_cn_moments']['names'] == mom['names']
        for k in posteriors.MOMENT_ARRAYS:
            assert np.array_equal(dist[j]['region_cn_moments'][k], on[i]['region_cn_moments'][k]), (i, k)
        for k in posteriors.MOMENT_STATS:
            assert dist[j]['stats'][k] == on[i]['stats'][k], (i, k)
    # the workflow (fit_restarts_distributed + collate): the arrays in the store, the stats in the stats table
    exp_file = str(tmp_path / 'experiment.pickle')
    with open(exp_file, 'wb') as f:
        pickle.dump(e, f)
    workflow.fit_model(exp_file, str(tmp_path / 'r.store'), dict(config, cn_regions=cn_regions, cn_region_moments=True), None, seeds=seeds)
    with pipeline._Store(str(tmp_path / 'r.store'), 'r') as st:
        stats = st['stats']
        for row, i in enumerate(stats['init_id']):
            for k in posteriors.MOMENT_ARRAYS:
                v = np.asarray(st['solutions/solution_%d/region_%s' % (i, k)])
                assert np.array_equal(v.reshape(shapes[k]), on[i]['region_cn_moments'][k]), (i, k)
            for k in posteriors.MOMENT_STATS:
                assert float(np.asarray(stats[k])[row]) == on[i]['stats'][k], (i, k)
    workflow.fit_model(exp_file, str(tmp_path / 'r0.store'), dict(config, cn_regions=cn_regions), None, seeds=seeds)
    with pipeline._Store(str(tmp_path / 'r0.store'), 'r') as st:
        assert not any('region_total_cn' in k or 'region_fraction' in k or 'region_length' in k for k in st.keys())
        assert not any(k in st['stats'].columns for k in posteriors.MOMENT_STATS)


def test_chunked_launch(hip):
    """A 2 000-segment run, and enough copies of one query to need two launches: every copy is identical."""
    from remixt_amd.restarts import RestartSet
    e = synthetic.make_experiment(2000, num_clones=3, max_copy_number=8, num_chains=5, seed=0)
    ps = synthetic.make_init_params(e, 4, 8)
    rs = RestartSet(e, ps, 8, num_clones=3, quiet=True, seeds=list(range(4)))
    try:
        rs.variational_update(1)
        b, m = rs.batch, rs.models[0]
        assert b.num_cn_states == 165
        feats = posteriors.moment_features(b.cn_classes)
        weights = np.asarray(m.l1, dtype=float)[None]
        cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
        whole = np.array([[a, z, f0, 0] for a, z in zip(cs, ce) for f0 in (0, 3)], dtype=np.int32)
        b.profile_reset(); b.profile_enable(1)
        out = b.region_moments_raw(0, 4, whole, feats, weights, 4)
        ms, launches = b.profile()['k_region_moments']; b.profile_enable(0)
        print('whole chains, 4 restarts x %d queries over %d segments: k_region_moments %.2f ms device in %d launches' % (len(whole), b.num_segments, ms, launches))
        assert out.shape == (4, len(whole), 14) and np.isfinite(out).all() and (ce - cs).max() > 300
        per = 14
        reps = (64 << 20) // (4 * per * 8 + 16) + 2
        short = np.array([[int(cs[1]), int(cs[1]) + 20, 3, 0]], dtype=np.int32)
        many = np.tile(short, (reps, 1))
        b.profile_reset(); b.profile_enable(1)
        big = b.region_moments_raw(0, 4, many, feats, weights, 4)
        launches = b.profile()['k_region_moments'][1]; b.profile_enable(0)
        assert launches >= 2
        assert (big == big[:, :1]).all() and np.array_equal(big[:, 0], b.region_moments_raw(0, 4, short, feats, weights, 4)[:, 0])
    finally:
        rs.close()
