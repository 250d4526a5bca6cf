"""Posterior path sampling on the device (rmx_sample_cn / k_sample_cn): exact agreement with the CPU twin, the
sampled distribution against the posterior marginals and adjacent joints, invariance to batching and grouping,
no side effects on the model, errors, and the bench-size workload."""
import numpy as np
import pytest

from remixt_amd import sampling, synthetic
from remixt_amd.restarts import tumour_ploidy_and_divergence
from tests import ffbs_twin
from tests import helpers as H

pytestmark = pytest.mark.gpu

# (segments, clones, max copy number): 165 / 355 states with three clones, 457 with four
GRIDS = [(60, 3, 8), (40, 3, 12), (24, 4, 6)]


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


def _fitted(hip, N, M, max_cn, chains=3, seed=0, sweeps=2, **kw):
    m, h, e = H.make_model(hip, N=N, M=M, max_cn=max_cn, chains=chains, seed=seed, **kw)
    if M == 4:      # (make_init_params describes three clones: the tumour depth split three ways)
        p = synthetic.make_init_params(e, 1, max_cn, num_clones=M)[0]
        h = np.array([p['h_normal']] + [p['h_tumour'] * f for f in (0.5, 0.3, 0.2)])
    H.attach(m, h)
    for _ in range(sweeps):
        m.variational_update()
    return m


def _model_state(m):
    mod = m.model
    out = dict((name, np.array(getattr(mod, name))) for name in H.STATE_ATTRS + H.DENSE_ATTRS + ['h'])
    for name in ('divergence_weight', 'hmm_log_norm_const', 'negbin_r_0', 'betabin_M_0'):
        out[name] = np.array(getattr(mod, name))
    return out


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_matches_cpu_twin(hip, N, M, max_cn):
    m = _fitted(hip, N, M, max_cn)
    b, r = m.model._batch, m.model._r
    assert b.num_cn_states == {8: 165, 12: 355, 6: 457}[max_cn]
    assert m.num_breakpoints > 0 and (np.asarray(m.breakpoint_idx) >= 0).any()
    f = np.array(m.model.framelogprob); T = np.array(m.model.log_transmat)
    K = 128
    seed = sampling.restart_seed(3, 1)
    got = b.sample_states(r, 1, K, [seed])[0]
    assert got.dtype == np.int16 and got.shape == (K, m.N1)
    want, flag = ffbs_twin.sample(f, T, seed, np.arange(K))
    assert flag.mean() < 1e-3, flag.mean()
    # after a flagged draw (u within 1e-9 of a CDF boundary) the rest of that path is not compared
    last_flag = np.where(flag.any(axis=1), m.N1 - 1 - np.argmax(flag[:, ::-1], axis=1), -1)
    cmp = np.arange(m.N1)[None, :] > last_flag[:, None]
    assert np.array_equal(got[cmp], want[cmp]), (b.info(12), np.argwhere(cmp & (got != want))[:5])
    cn = m.model.sample_cn(K, seed)
    assert cn.shape == (K, m.N1, b.num_clones, 2) and cn.dtype == np.int64
    assert np.array_equal(cn, b.states_to_cn(got))


def test_distribution(hip):
    m = _fitted(hip, 30, 3, 8, sweeps=3)
    K = 4096
    st = m.model._batch.sample_states(m.model._r, 1, K, [99]).astype(np.int64)[0]
    post = np.array(m.model.posterior_marginals)
    N, S = post.shape
    freq = np.zeros((N, S))
    for n in range(N):
        freq[n] = np.bincount(st[:, n], minlength=S) / K
    tol = 6 * np.sqrt(post * (1 - post) / K) + 2. / K
    assert (np.abs(freq - post) <= tol).all(), np.abs(freq - post).max()
    joint = np.array(m.model.joint_posterior_marginals)
    for n in range(N - 1):
        pf = np.bincount(st[:, n] * S + st[:, n + 1], minlength=S * S).reshape(S, S) / K
        tol = 6 * np.sqrt(joint[n] * (1 - joint[n]) / K) + 2. / K
        assert (np.abs(pf - joint[n]) <= tol).all(), (n, np.abs(pf - joint[n]).max())


def test_invariance(hip):
    from remixt_amd.restarts import RestartGroups, RestartSet
    e = synthetic.make_experiment(80, num_clones=3, max_copy_number=4, num_chains=3, seed=4)
    ps = synthetic.make_init_params(e, 4, 4)
    rs = RestartSet(e, ps, 4, num_clones=3, quiet=True, seeds=list(range(4)))
    # (read counts masked out: a posterior with many likely paths, so that different seeds can tell)
    mod0 = rs.models[0].model
    mod0.total_likelihood_mask = np.zeros(mod0.num_segments, dtype=int)
    mod0.allele_likelihood_mask = np.zeros(mod0.num_segments, dtype=int)
    rs.variational_update(2)
    b = rs.batch
    assert np.array(rs.models[0].model.posterior_marginals).max(axis=1).min() < 0.9
    seeds = [sampling.restart_seed(1, i) for i in range(4)]
    full = b.sample_states(0, 4, 48, seeds)
    for r in range(4):
        assert np.array_equal(b.sample_states(r, 1, 48, [seeds[r]])[0], full[r])
    assert np.array_equal(b.sample_states(1, 2, 48, seeds[1:3]), full[1:3])
    assert np.array_equal(b.sample_states(0, 4, 16, seeds), full[:, :16])      # a sample's path does not depend on how many are drawn
    other = b.sample_states(0, 4, 48, [s + 1 for s in seeds])
    assert not np.array_equal(other, full)
    assert not np.array_equal(full[0, 0], full[0, 1]) or not np.array_equal(full[0, 2], full[0, 3])
    per_set = rs.sample_cn(48, seed=1)
    rs.close()
    groups = RestartGroups(e, ps, 4, groups=2, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    single = RestartGroups(e, ps, 4, groups=1, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    for g in (groups, single):
        g.variational_update(2)
    a, c = groups.sample_cn(48, seed=1), single.sample_cn(48, seed=1)
    for r in range(4):
        assert np.array_equal(a[r], c[r])
        assert a[r].shape == per_set[r].shape
    groups.close(); single.close()


def test_no_side_effects(hip):
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    before = _model_state(m1)
    vit0 = np.zeros((m1.N1, 3, 2), dtype=int); m1.model.infer_cn(vit0)
    m1.model.sample_cn(64, 5)
    m1.sample_cn(8, 6)
    after = _model_state(m1)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    # a fit continued after the sample call equals one without it
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
    with pytest.raises(ValueError, match='update_p_cn'):
        b.sample_states(r, 1, 4, [0])
    assert bpmodel.last_error_restarts() == [r]
    m.variational_update()
    for args in ((r, 1, 0, [0]), (r + 1, 1, 4, [0]), (-1, 1, 4, [0]), (r, 0, 4, [])):      # RMX_EARG
        with pytest.raises(ValueError, match='^bad argument: bad argument$'):
            b.sample_states(*args)
        assert bpmodel.last_error_restarts() == []
    with pytest.raises(ValueError, match='one seed per restart'):
        b.sample_states(r, 1, 4, [0, 1])
    assert b.sample_states(r, 1, 4, [0]).shape == (1, 4, m.N1)
    from oracle import oracle
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError):
        mo.sample_cn(4)


def test_full_size(hip):
    from remixt_amd.restarts import RestartSet
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=8, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, 16, 8)
    rs = RestartSet(e, ps, 8, num_clones=3, quiet=True, seeds=list(range(16)))
    try:
        rs.variational_update(1)
        assert rs.batch.num_cn_states == 165
        st = rs.batch.sample_states(0, 16, 64, [sampling.restart_seed(0, i) for i in range(16)])
        assert st.shape == (16, 64, rs.batch.num_segments)
        assert st.min() >= 0 and st.max() < 165
    finally:
        rs.close()


def _pipeline_case():
    from remixt_amd.analysis import pipeline
    e = synthetic.make_experiment(600, num_clones=3, max_copy_number=4, num_chains=5, seed=14)
    config = {'max_copy_number': 4, 'h_normal': float(e.h[0]), 'h_tumour': float(e.h[1:].sum()), 'tumour_mix_fractions': [0.45, 0.3],
              'divergence_weights': [1e-6, 1e-8], 'num_em_iter': 2, 'num_update_iter': 3, 'min_ploidy': None, 'max_ploidy': None}
    init_params, _, _ = pipeline.generate_init_params(e, config)
    return e, config, init_params


def _same_results(a, b):
    assert sorted(a) == sorted(b)
    for i in a:
        assert sorted(a[i]) == sorted(b[i]) and sorted(a[i]['stats']) == sorted(b[i]['stats'])
        for k, v in a[i].items():
            if k == 'stats':
                for sk, sv in v.items():
                    assert (sv == b[i]['stats'][sk]) or (sv != sv and b[i]['stats'][sk] != b[i]['stats'][sk]), (i, sk)
            elif k == 'brk_cn':
                assert all(np.array_equal(v[bk], b[i][k][bk]) for bk in v)
            else:
                assert np.array_equal(np.asarray(v), np.asarray(b[i][k])), (i, k)


def test_pipeline_cn_samples(hip, tmp_path):
    from remixt_amd import workflow
    from remixt_amd.analysis import pipeline
    from remixt_amd.restarts import RestartSet
    import pickle
    e, config, init_params = _pipeline_case()
    ids = sorted(init_params)
    seeds = [100 + i for i in ids]
    base = pipeline.fit_restarts(e, init_params, config, seeds=seeds, groups=1)
    off = pipeline.fit_restarts(e, init_params, dict(config, num_cn_samples=0), seeds=seeds, groups=1)
    _same_results(base, off)
    K, seed = 32, 7
    on = pipeline.fit_restarts(e, init_params, dict(config, num_cn_samples=K, cn_sample_seed=seed), seeds=seeds, groups=1)
    # host recomputation from sample_cn of the same fit
    rs = RestartSet(e, [init_params[i] for i in ids], 4, num_clones=3, quiet=True, seeds=seeds, **pipeline._model_kwargs(e, config))
    rs.fit(config['num_em_iter'], config['num_update_iter'])
    samples = rs.sample_cn(K, seed, init_ids=ids)
    rs.close()
    l = np.asarray(e.l)
    for j, i in enumerate(ids):
        res = on[i]
        assert np.array_equal(res['cn'], base[i]['cn'])
        agree, state = res['cn_sample_agreement'], res['cn_state_agreement']
        assert agree.shape == (len(e.l), 3) and state.shape == (len(e.l),)
        assert (agree >= 0).all() and (agree <= 1).all() and (state >= 0).all() and (state <= 1).all() and (state <= agree.min(axis=1)).all()
        st = res['stats']
        for name in ('ploidy', 'proportion_divergent'):
            assert st[name + '_q05'] <= st[name + '_q50'] <= st[name + '_q95']
        smp = samples[j]
        assert smp.shape == (K, len(e.l), 3, 2)
        eq = (smp == res['cn'][None]).all(axis=3)
        assert np.array_equal(agree, eq.mean(axis=0)) and np.array_equal(state, eq.all(axis=2).mean(axis=0))
        ploidy, prop = [], []
        for k in range(K):
            pl, div = tumour_ploidy_and_divergence(smp[k], l)
            ploidy.append(pl); prop.append((div.T * l).sum() / (2. * l.sum()))
        for name, v in (('ploidy', ploidy), ('proportion_divergent', prop)):
            q = np.quantile(v, [0.05, 0.5, 0.95])
            assert np.allclose([st[name + '_q05'], st[name + '_q50'], st[name + '_q95']], q, rtol=1e-12, atol=0)
    # one restart through pipeline.fit: the same stream as its batched form
    one = pipeline.fit(e, init_params[ids[1]], dict(config, num_cn_samples=K, cn_sample_seed=seed), quiet=True, init_id=ids[1])
    assert one['cn_sample_agreement'].shape == (len(e.l), 3) and 'ploidy_q50' in one['stats']
    # the workflow (fit_restarts_distributed + collate): the summary in the record, the arrays in the store
    exp_file = str(tmp_path / 'experiment.pickle')
    with open(exp_file, 'wb') as f:
        pickle.dump(e, f)
    workflow.fit_model(exp_file, str(tmp_path / 'r.store'), dict(config, num_cn_samples=K, cn_sample_seed=seed), None)
    with pipeline._Store(str(tmp_path / 'r.store'), 'r') as st:
        stats = st['stats']
        for k in sampling.SUMMARY_STATS:
            assert k in stats.columns
        for i in sorted(stats['init_id']):
            a = st['solutions/solution_%d/cn_sample_agreement' % i]
            assert a.shape == (len(e.l), 3) and ((a.values >= 0) & (a.values <= 1)).all()
            assert len(st['solutions/solution_%d/cn_state_agreement' % i]) == len(e.l)
    workflow.fit_model(exp_file, str(tmp_path / 'r0.store'), config, None)
    with pipeline._Store(str(tmp_path / 'r0.store'), 'r') as st:
        assert not any('cn_sample_agreement' in k for k in st.keys()) and 'ploidy_q50' not in st['stats'].columns
