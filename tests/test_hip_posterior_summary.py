"""Exact posterior summaries on the device (rmx_posterior_summary / k_posterior_summary): projection, row statistics and
arg-max against the numpy twin on the posterior read back from the same device, crafted rows, tiles that mix state classes,
invariance to batching, nullable outputs, no side effects, errors, the model / container / pipeline layers, and the bench size.

Tolerances.  Projection: device and numpy each form an S-term floating-point sum, error at most (S + 8) 2^-53 sum|p w| in any
order, so element-wise 4 S 2^-53 (|post| @ |W|).  Entropy: (S + 8) 2^-52 sum|p log p| (log within 3 ulp on the device, 1 ulp in
numpy, and the two sums).  Row maximum, gathered entry and arg-max: bit-exact."""
import numpy as np
import pytest

from remixt_amd import posteriors, sampling, synthetic
from tests import helpers as H
from tests import posterior_twin as twin

pytestmark = pytest.mark.gpu

# (segments, clones, max copy number): 165 / 355 / 457 states (rows padded to 168 / 360 / 464); 38 / 21 / 21 model segments: no
# multiple of the 16-segment tile, the first more than two tiles
GRIDS = [(37, 3, 8), (21, 3, 12), (19, 4, 6)]
QS = [1, 16, 17, 64, 256]
U = 2. ** -53


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


def _fitted(hip, N, M, max_cn, chains=3, seed=0, sweeps=2, experiment=None, masked=False):
    m, h, e = H.make_model(hip, N=N, M=M, max_cn=max_cn, chains=chains, seed=seed, experiment=experiment)
    if M == 4:      # (make_init_params describes three clones: the tumour depth split three ways)
        p = synthetic.make_init_params(e, 1, max_cn, num_clones=M)[0]
        h = np.array([p['h_normal']] + [p['h_tumour'] * f for f in (0.5, 0.3, 0.2)])
    H.attach(m, h)
    if masked:      # (read counts masked out: a posterior spread over many states)
        m.model.total_likelihood_mask = np.zeros(m.model.num_segments, dtype=int)
        m.model.allele_likelihood_mask = np.zeros(m.model.num_segments, dtype=int)
    for _ in range(sweeps):
        m.variational_update()
    return m


@pytest.fixture(scope='module')
def fitted(hip):
    """The three grids after two real sweeps (the pad columns hold what the sweep kernels left), built once."""
    return dict(((N, M, c), _fitted(hip, N, M, c)) for N, M, c in GRIDS)


def _check_projection(proj, post, W, seg_class, tag=''):
    S = post.shape[1]
    want = twin.project(post, W, seg_class)
    tol = 4 * S * U * twin.projection_scale(post, W, seg_class)
    err = np.abs(proj - want)
    print('%s projection: max err %.3e, max err / tol %.3f' % (tag, err.max(), (err / np.maximum(tol, 1e-300)).max()))
    assert (err <= tol).all(), (tag, float(err.max()), np.argwhere(err > tol)[:5])


def _check_stats(stats, amax, post, states, tag=''):
    S = post.shape[1]
    _, want, want_am = twin.summary(post, states=states)
    tol = (S + 8) * 2. ** -52 * twin.entropy_scale(post)
    err = np.abs(stats[:, 1] - want[:, 1])
    print('%s entropy: max err %.3e, max err / tol %.3f' % (tag, err.max(), (err / np.maximum(tol, 1e-300)).max()))
    assert np.isfinite(stats).all() and (err <= tol).all(), (tag, float(err.max()))
    assert np.array_equal(stats[:, 0], want[:, 0]), tag
    assert np.array_equal(stats[:, 2], want[:, 2]), tag
    assert amax.dtype == np.int16 and np.array_equal(amax, want_am), tag


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_matches_twin(hip, fitted, N, M, max_cn):
    m = fitted[(N, M, max_cn)]
    b, r = m.model._batch, m.model._r
    S = b.num_cn_states
    assert S == {8: 165, 12: 355, 6: 457}[max_cn] and S % 4 and b.num_segments % 16
    post = b.get_array(r, 'posterior_marginals')
    rng = np.random.RandomState(N)
    states = rng.randint(0, S, size=b.num_segments)
    C_ = b.cn_classes.shape[0]
    b.profile_reset(); b.profile_enable(1)
    for Q in QS:
        W = rng.normal(size=(C_, S, Q))
        proj, stats, amax = b.posterior_summary_raw(r, 1, weights=W, states=states[None])
        assert proj.shape == (1, b.num_segments, Q) and stats.shape == (1, b.num_segments, 3) and amax.shape == (1, b.num_segments)
        _check_projection(proj[0], post, W, b.seg_class, 'S %d Q %d' % (S, Q))
        _check_stats(stats[0], amax[0], post, states, 'S %d Q %d' % (S, Q))
    prof = b.profile(); b.profile_enable(0)
    assert prof['k_posterior_summary'][1] == len(QS) and prof['k_posterior_summary'][0] > 0
    # a (S, Q) table serves every class; the model-level conveniences
    W2 = rng.normal(size=(S, 5))
    p2 = m.model.posterior_project(W2)
    assert p2.shape == (b.num_segments, 5)
    _check_projection(p2, post, np.repeat(W2[None], C_, axis=0), b.seg_class, 'posterior_project')
    # the posterior is unchanged by all of it
    assert np.array_equal(post, b.get_array(r, 'posterior_marginals'))


def test_crafted_rows(hip, fitted):
    m = fitted[GRIDS[0]]
    b, r = m.model._batch, m.model._r
    S, N = b.num_cn_states, b.num_segments
    rng = np.random.RandomState(5)
    post = rng.dirichlet(np.full(S, 0.2), size=N)
    post[0] = 0.; post[0, 7] = 1.                                       # one-hot
    post[1] = 0.                                                        # all zero
    post[2] = 0.4 / (S - 2); post[2, 3] = 0.3; post[2, 150] = 0.3       # the maximum twice
    post[3] = 0.; post[3, 10] = 0.5; post[3, 11] = 5e-324; post[3, 12] = 1e-310; post[3, 164] = 2e-308      # subnormal entries
    post[17] = 0.; post[17, S - 1] = 1.                                 # one-hot at the last real column, second tile
    b.set_array(r, 'posterior_marginals', post)
    assert np.array_equal(b.get_array(r, 'posterior_marginals'), post)
    for Q in (1, 17, 64):
        W = rng.normal(size=(b.cn_classes.shape[0], S, Q))
        states = rng.randint(0, S, size=N)
        proj, stats, amax = b.posterior_summary_raw(r, 1, weights=W, states=states[None])
        proj, stats, amax = proj[0], stats[0], amax[0]
        assert np.array_equal(proj[0], W[b.seg_class[0], 7]) and stats[0, 0] == 1. and stats[0, 1] == 0. and amax[0] == 7
        assert np.array_equal(proj[17], W[b.seg_class[17], S - 1]) and stats[17, 1] == 0. and amax[17] == S - 1
        assert (proj[1] == 0).all() and (stats[1] == 0).all() and amax[1] == 0
        assert amax[2] == 3 and stats[2, 0] == 0.3
        assert np.isfinite(stats[3, 1]) and stats[3, 1] > 0 and amax[3] == 10
        _check_projection(proj, post, W, b.seg_class, 'crafted Q %d' % Q)
        _check_stats(stats, amax, post, states, 'crafted Q %d' % Q)


def test_mixed_classes_in_a_tile(hip):
    m, h, e = H.make_model(hip, N=40, M=3, max_cn=4, chains=3)
    M = 3
    classes, _ = m._state_tables(M)
    classes = np.repeat(classes[:1], 2, axis=0)
    classes[1, :, 0, :] = (1, 0)
    N = m.N1
    assert N >= 40
    seg_class = (np.arange(N) % 2).astype(np.int32)                      # 0, 1, 0, 1, ...
    brk_states = m.create_brk_states(M, m.max_copy_number, m.max_copy_number_diff)
    b = hip.RemixtBatch(M, N, m.num_breakpoints, m.normal_contamination, classes, seg_class, brk_states, np.asarray(h, dtype=float)[None],
                        m.l1, m.x1[:, 2].copy(), m.x1[:, 0:2].copy(), m.is_telomere, m.breakpoint_idx, m.breakpoint_orient,
                        m.transition_log_prob, [m.divergence_weight])
    try:
        S = b.num_cn_states
        rng = np.random.RandomState(8)
        post = rng.dirichlet(np.full(S, 0.3), size=N)
        b.set_array(0, 'posterior_marginals', post)
        states = rng.randint(0, S, size=N)
        for Q in (3, 17):
            W = rng.normal(size=(2, S, Q))
            W[1] += 3.                                                   # the classes' tables differ everywhere
            proj, stats, amax = b.posterior_summary_raw(0, 1, weights=W, states=states[None])
            _check_projection(proj[0], post, W, seg_class, 'mixed Q %d' % Q)
            _check_stats(stats[0], amax[0], post, states, 'mixed')
            # (a kernel that took one class for the whole tile would miss by the shift of 3)
            wrong = twin.project(post, W, np.zeros(N, dtype=int))
            assert np.abs(proj[0][1::2] - wrong[1::2]).min() > 1.
        # the feature tables of the two classes: the normal clone's total and LOH differ
        s = posteriors.batch_summaries(b, 0, 1)[0]
        assert np.allclose(s['total_cn_mean'][:, 0], np.where(seg_class == 0, 2., 1.), rtol=1e-12, atol=0)      # (times the row sum)
        assert (s['p_loh'][0::2] == 0).all() and (s['p_loh'][1::2] > 0).all() and s['p_loh'].max() <= 1 + 1e-12      # (a normal row of (1, 1) rules LOH out)
    finally:
        b.close()


def test_batching_invariance_and_containers(hip):
    from remixt_amd.restarts import DatasetGroups, RestartGroups, RestartSet
    e = synthetic.make_experiment(37, num_clones=3, max_copy_number=8, num_chains=3, seed=1)
    ps = synthetic.make_init_params(e, 5, 8)
    rs = RestartSet(e, ps, 8, num_clones=3, quiet=True, seeds=list(range(5)))
    rs.variational_update(2)
    b = rs.batch
    S, N = b.num_cn_states, b.num_segments
    rng = np.random.RandomState(2)
    W = rng.normal(size=(b.cn_classes.shape[0], S, 17))
    states = rng.randint(0, S, size=(5, N))
    full = b.posterior_summary_raw(0, 5, weights=W, states=states)
    assert not np.array_equal(full[0][0], full[0][1])                  # the restarts differ
    for r in range(5):
        one = b.posterior_summary_raw(r, 1, weights=W, states=states[r:r + 1])
        for a, f in zip(one, full):
            assert np.array_equal(a[0], f[r])
    part = b.posterior_summary_raw(1, 2, weights=W, states=states[1:3])
    for a, f in zip(part, full):
        assert np.array_equal(a, f[1:3])
    # containers: one call per batch, every restart equal to its model's own summary
    res = rs.results()
    per_set = rs.posterior_summary(cn=[x['cn'] for x in res], marginals=True)
    assert len(per_set) == 5
    for r, mod in enumerate(rs.models):
        cn_model = np.zeros((N, 3, 2), dtype=int); mod.model.infer_cn(cn_model)
        own = mod.posterior_summary(cn=cn_model, marginals=True)
        assert sorted(own) == sorted(per_set[r])
        for k in own:
            assert np.array_equal(own[k], per_set[r][k]), k
    assert 'cn_posterior_prob' not in rs.posterior_summary()[0]
    rs.close()
    groups = RestartGroups(e, ps, 8, groups=2, num_clones=3, quiet=True, seeds=list(range(5)))
    groups.variational_update(1)
    out = groups.posterior_summary()
    assert len(out) == 5
    for s, mod in zip(out, groups.models):
        own = mod.posterior_summary()
        for k in own:
            assert np.array_equal(own[k], s[k]), k
    groups.close()
    dg = DatasetGroups([e, e], [ps[:2], ps[2:4]], 8, seeds=[[0, 1], [2, 3]], num_clones=3, quiet=True)
    dg.variational_update(1)
    res = dg.results_by_dataset()
    out = dg.posterior_summary(cn=[[x['cn'] for x in part] for part in res])
    assert len(out) == 4
    for s, mod in zip(out, dg.models):
        own = mod.posterior_summary()
        for k in own:
            assert np.array_equal(own[k], s[k]), k
        assert 'cn_posterior_prob' in s
    dg.close()


def test_nullable_outputs(hip, fitted):
    m = fitted[GRIDS[1]]
    b, r = m.model._batch, m.model._r
    S, N = b.num_cn_states, b.num_segments
    rng = np.random.RandomState(3)
    W = rng.normal(size=(b.cn_classes.shape[0], S, 17))
    states = rng.randint(0, S, size=(1, N))
    proj, stats, amax = b.posterior_summary_raw(r, 1, weights=W, states=states)
    p, s, a = b.posterior_summary_raw(r, 1, weights=W, want_stats=False, want_argmax=False)
    assert s is None and a is None and np.array_equal(p, proj)
    p, s, a = b.posterior_summary_raw(r, 1, states=states, want_argmax=False)
    assert p is None and a is None and np.array_equal(s, stats)
    p, s, a = b.posterior_summary_raw(r, 1, want_stats=False)
    assert p is None and s is None and np.array_equal(a, amax)
    p, s, a = b.posterior_summary_raw(r, 1, weights=W, want_stats=False)
    assert s is None and np.array_equal(p, proj) and np.array_equal(a, amax)
    p, s, a = b.posterior_summary_raw(r, 1, weights=W)               # no states: the third statistic is 0
    assert np.array_equal(s[..., :2], stats[..., :2]) and (s[..., 2] == 0).all() and np.array_equal(p, proj)


def _model_state(m):
    mod = m.model
    out = dict((name, np.array(getattr(mod, name))) for name in H.STATE_ATTRS + H.DENSE_ATTRS + ['h'])
    for name in ('divergence_weight', 'hmm_log_norm_const', 'negbin_r_0', 'betabin_M_0'):
        out[name] = np.array(getattr(mod, name))
    return out


def test_no_side_effects(hip):
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    before = _model_state(m1)
    b = m1.model._batch
    W = np.random.RandomState(0).normal(size=(b.num_cn_states, 33))
    b.posterior_summary_raw(m1.model._r, 1, weights=W, states=np.zeros((1, b.num_segments), dtype=int))
    m1.posterior_summary(marginals=True)
    after = _model_state(m1)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    for m in (m1, m2):
        m.variational_update()
    s1, s2 = _model_state(m1), _model_state(m2)
    for k in s1:
        assert np.array_equal(s1[k], s2[k], equal_nan=True), k
    assert m1.model.calculate_elbo() == m2.model.calculate_elbo()


def test_errors(hip):
    m = _fitted(hip, 30, 3, 3, sweeps=1)
    b, r = m.model._batch, m.model._r
    S, N = b.num_cn_states, b.num_segments
    W = np.ones((S, 4))
    ok_states = np.zeros((1, N), dtype=int)
    bad_hi = ok_states.copy(); bad_hi[0, N - 1] = S
    bad_lo = ok_states.copy(); bad_lo[0, 0] = -1
    cases = [
        dict(r0=r, nr=1, weights=np.ones((S, 0))),                       # Q = 0 with weights
        dict(r0=r, nr=1, weights=np.ones((S, 257))),                     # Q = 257
        dict(r0=r + 1, nr=1, weights=W), dict(r0=-1, nr=1, weights=W), dict(r0=r, nr=0, weights=W), dict(r0=r, nr=2, weights=W),
        dict(r0=r, nr=1, weights=W, states=bad_hi), dict(r0=r, nr=1, states=bad_hi), dict(r0=r, nr=1, weights=W, states=bad_lo),
        dict(r0=r, nr=1, want_stats=False, want_argmax=False),           # nothing requested
    ]
    for kw in cases:
        with pytest.raises(ValueError, match='bad argument'):
            b.posterior_summary_raw(kw.pop('r0'), kw.pop('nr'), **kw)
        assert hip.last_error_restarts() == []
    with pytest.raises(ValueError, match='weights must have shape'):
        b.posterior_summary_raw(r, 1, weights=np.ones((S + 1, 4)))
    with pytest.raises(ValueError, match='states must have shape'):
        b.posterior_summary_raw(r, 1, states=np.zeros((1, N + 1), dtype=int))
    # the batch is usable afterwards
    post = b.get_array(r, 'posterior_marginals')
    proj, stats, amax = b.posterior_summary_raw(r, 1, weights=W, states=ok_states)
    _check_projection(proj[0], post, np.repeat(W[None], b.cn_classes.shape[0], axis=0), b.seg_class, 'after errors')
    _check_stats(stats[0], amax[0], post, ok_states[0], 'after errors')
    m.variational_update()
    from oracle import oracle
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError):
        mo.posterior_summary()


@pytest.fixture(scope='module')
def end_to_end(hip):
    """60 segments with a boundary shared by two breakpoints (the segment remap inserts a segment), read counts masked (a
    posterior spread over many states), three sweeps."""
    e = synthetic.make_experiment(60, num_clones=3, max_copy_number=8, num_chains=3, seed=3)
    e.breakpoints = H.add_shared_boundary_breakpoints(e)
    return _fitted(hip, 60, 3, 8, sweeps=3, experiment=e, masked=True), e


def test_end_to_end(hip, end_to_end):
    m, e = end_to_end
    b, r = m.model._batch, m.model._r
    S, N1 = b.num_cn_states, b.num_segments
    fwd = np.asarray(m.seg_fwd_remap)
    assert N1 > len(e.l) and not np.array_equal(fwd, np.arange(len(fwd)))
    cn_model = np.zeros((N1, 3, 2), dtype=int); m.model.infer_cn(cn_model)
    s = m.posterior_summary(cn=cn_model, marginals=True)
    post = b.get_array(r, 'posterior_marginals')
    assert s['cn_marginals'].shape == (len(e.l), 3, 2, 9)
    dev = np.abs(s['cn_marginals'].sum(axis=3) - 1.)
    print('cn_marginals: max |sum - 1| %.3e (bound %.3e)' % (dev.max(), 4 * S * U))
    assert (dev <= 4 * S * U).all()
    W, lay = posteriors.feature_matrix(b.cn_classes, marginals=True)
    want = twin.project(post, W, b.seg_class)
    tol = 4 * S * U * twin.projection_scale(post, W, b.seg_class)
    assert (np.abs(s['total_cn_mean'] - want[:, lay['tot']][fwd]) <= tol[:, lay['tot']][fwd]).all()
    states = posteriors.cn_to_states(cn_model, b.cn_classes, b.seg_class)
    assert np.array_equal(b.states_to_cn(states), cn_model)
    assert np.array_equal(s['cn_posterior_prob'], post[np.arange(N1), states][fwd])
    cn_exp, _ = m.optimal_cn()
    assert np.array_equal(cn_exp, cn_model[fwd])
    # experiment order: every array is the model-order one through seg_fwd_remap
    raw = posteriors.batch_summaries(b, r, 1, states=states[None], marginals=True)[0]
    assert sorted(raw) == sorted(s)
    for k in raw:
        assert s[k].shape[0] == len(e.l) and np.array_equal(s[k], raw[k][fwd]), k
    assert np.array_equal(s['cn_mpm'], b.cn_classes[b.seg_class, post.argmax(axis=1)][fwd])
    assert (s['cn_posterior_prob'] <= s['cn_posterior_max']).all()


def test_against_the_sampler(hip, end_to_end):
    """The sample means of ploidy and proportion divergent over 4 096 posterior paths against the exact expectations: within 6
    standard errors, the standard error from the samples' own variance (the sampler alone sets the margin)."""
    m, e = end_to_end
    K = 4096
    samples = m.sample_cn(K, sampling.restart_seed(11, 0))
    ploidy, prop = sampling.ploidy_and_divergence_samples(samples, e.l)
    st = posteriors.summary_stats(m.posterior_summary(), e.l)
    for name, v in (('ploidy_posterior_mean', ploidy), ('proportion_divergent_posterior_mean', prop)):
        se = v.std(ddof=1) / np.sqrt(K)
        print('%s: exact %.6f, sample mean %.6f, standard error %.2e' % (name, st[name], v.mean(), se))
        assert abs(v.mean() - st[name]) <= 6 * se, name


def _pipeline_case():
    from remixt_amd.analysis import pipeline
    e = synthetic.make_experiment(600, num_clones=3, max_copy_number=4, num_chains=5, seed=14)
    config = {'max_copy_number': 4, 'h_normal': float(e.h[0]), 'h_tumour': float(e.h[1:].sum()), 'tumour_mix_fractions': [0.45, 0.3],
              'divergence_weights': [1e-6, 1e-8], 'num_em_iter': 2, 'num_update_iter': 3, 'min_ploidy': None, 'max_ploidy': None}
    init_params, _, _ = pipeline.generate_init_params(e, config)
    return e, config, init_params


def _check_result(res, N, M=3):
    for k in posteriors.COMPACT_ARRAYS:
        assert res[k].shape == ((N, M) if k.startswith('total_cn') else (N,)), k
        assert np.isfinite(res[k]).all(), k
    # (a probability is an S-term sum of a normalised row: it may pass 1 by rounding, never by 1e-12)
    for k in ('cn_posterior_prob', 'cn_posterior_max', 'p_subclonal', 'p_loh', 'p_hdel'):
        assert (res[k] >= 0).all() and (res[k] <= 1 + 1e-12).all(), k
    assert (res['cn_posterior_prob'] <= res['cn_posterior_max']).all()
    assert (res['cn_posterior_entropy'] >= 0).all() and (res['total_cn_sd'] >= 0).all() and (res['total_cn_mean'] >= 0).all()
    for k in posteriors.SUMMARY_STATS:
        assert np.isfinite(res['stats'][k]) and res['stats'][k] >= 0


def test_pipeline(hip, tmp_path):
    import pickle
    from remixt_amd import workflow
    from remixt_amd.analysis import pipeline
    e, config, init_params = _pipeline_case()
    ids = sorted(init_params)
    seeds = [100 + i for i in ids]
    N = len(e.l)
    base = pipeline.fit_restarts(e, init_params, config, seeds=seeds, groups=1)
    off = pipeline.fit_restarts(e, init_params, dict(config, cn_posterior_summary=False), seeds=seeds, groups=1)
    on = pipeline.fit_restarts(e, init_params, dict(config, cn_posterior_summary=True), seeds=seeds, groups=1)
    new_keys = set(posteriors.COMPACT_ARRAYS)
    for i in ids:
        assert sorted(off[i]) == sorted(base[i]) and sorted(off[i]['stats']) == sorted(base[i]['stats'])
        assert not (new_keys & set(base[i])) and not (set(posteriors.SUMMARY_STATS) & set(base[i]['stats']))
        assert set(on[i]) == set(base[i]) | new_keys
        assert set(on[i]['stats']) == set(base[i]['stats']) | set(posteriors.SUMMARY_STATS)
        assert np.array_equal(on[i]['cn'], base[i]['cn']) and on[i]['stats']['elbo'] == base[i]['stats']['elbo']
        _check_result(on[i], N)
    one = pipeline.fit(e, init_params[ids[1]], dict(config, cn_posterior_summary=True), quiet=True, init_id=ids[1])
    _check_result(one, N)
    exp_file = str(tmp_path / 'experiment.pickle')
    with open(exp_file, 'wb') as f:
        pickle.dump(e, f)
    workflow.fit_model(exp_file, str(tmp_path / 'r.store'), dict(config, cn_posterior_summary=True), None)
    with pipeline._Store(str(tmp_path / 'r.store'), 'r') as st:
        stats = st['stats']
        for k in posteriors.SUMMARY_STATS:
            assert k in stats.columns
        for i in sorted(stats['init_id']):
            for k in posteriors.COMPACT_ARRAYS:
                a = st['solutions/solution_%d/%s' % (i, k)]
                assert a.shape == ((N, 3) if k.startswith('total_cn') else (N,)), k
            assert 'solutions/solution_%d/cn_sample_agreement' % i not in st.keys()


def test_bench_size(hip):
    """50 000 segments x 165 states, 2 restarts: the compact set, and a 256-column projection whose 207 MB of output goes
    through the 64 MiB staging buffer in segment chunks (rows on both sides of the chunk boundaries against numpy)."""
    from remixt_amd.restarts import RestartSet
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=8, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, 2, 8)
    rs = RestartSet(e, ps, 8, num_clones=3, quiet=True, seeds=[0, 1])
    try:
        rs.variational_update(1)
        b = rs.batch
        S, N = b.num_cn_states, b.num_segments
        assert S == 165
        cn_all, _ = b.infer_cn_batch(0, 2)
        out = rs.posterior_summary(cn=[c[m.seg_fwd_remap] for c, m in zip(cn_all, rs.models)])
        for s in out:
            for k in posteriors.COMPACT_ARRAYS:
                assert s[k].shape == ((len(e.l), 3) if k.startswith('total_cn') else (len(e.l),)) and np.isfinite(s[k]).all(), k
            for k in ('cn_posterior_prob', 'cn_posterior_max', 'p_subclonal', 'p_loh', 'p_hdel'):
                assert (s[k] >= 0).all() and (s[k] <= 1 + 1e-12).all(), k
        W = np.random.RandomState(0).normal(size=(S, 256))
        proj, _, _ = b.posterior_summary_raw(0, 2, weights=W, want_stats=False, want_argmax=False)
        per_seg = 256 * 8
        ncap = ((64 << 20) // (2 * per_seg)) // 16 * 16
        assert 16 <= ncap < N
        post = b.get_array(1, 'posterior_marginals')
        rows = np.unique(np.concatenate([np.arange(0, 20), np.arange(ncap - 20, ncap + 20), np.arange(2 * ncap - 20, 2 * ncap + 20), np.arange(N - 20, N)]))
        Wc = np.repeat(W[None], b.cn_classes.shape[0], axis=0)
        _check_projection(proj[1][rows], post[rows], Wc, b.seg_class[rows], 'bench size, restart 1')
        assert np.isfinite(proj).all() and np.abs(proj[0] - proj[1]).max() > 0
    finally:
        rs.close()
