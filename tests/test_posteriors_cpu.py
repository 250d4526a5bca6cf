"""Host side of the exact posterior summaries (remixt_amd/posteriors.py): the weight tables against brute-force loops with the
reference's definitions, the path -> state inverse, the named arrays and whole-genome expectations on an enumerable
posterior, and the distributed result record with the option on and off."""
import numpy as np
import pytest

from remixt_amd import posteriors, restarts, synthetic
from remixt_amd.cn_model import create_cn_states
from remixt_amd.restarts import tumour_ploidy_and_divergence
from tests import posterior_twin as twin
from tests.test_cn_samples_records_cpu import _fake_result


def _classes(M=3, cn_max=2, normals=((1, 1), (1, 0), (2, 0))):
    grid = np.asarray(create_cn_states(M, 2, cn_max, 1))
    classes = np.repeat(grid[None], len(normals), axis=0).astype(np.int64)
    classes[:, :, 0, :] = np.asarray(normals)[:, None, :]
    return classes


def test_feature_matrix_against_loops():
    classes = _classes()
    C, S, M, _ = classes.shape
    seg_class = np.array([0, 1, 2, 1, 0, 2, 2])
    dense = classes[seg_class]                                  # (N, S, M, 2) as the reference holds it
    # bpmodel.pyx:505-507
    nas = np.sum(dense[:, :, 1:, :].max(axis=-2) != dense[:, :, 1:, :].min(axis=-2), axis=-1)
    is_hdel = np.all(dense == 0, axis=(-2, -1)) * 1
    is_loh = np.any(dense.sum(axis=-2) == 0, axis=-1) * 1
    for marg in (False, True):
        W, lay = posteriors.feature_matrix(classes, marginals=marg)
        cmax = int(classes.max())
        assert W.shape == (C, S, 2 * M + 4 + (M * 2 * (cmax + 1) if marg else 0)) and lay['Q'] == W.shape[2]
        for n, c in enumerate(seg_class):
            for s in range(S):
                row = W[c, s]
                for m in range(M):
                    t = dense[n, s, m, 0] + dense[n, s, m, 1]
                    assert row[lay['tot']][m] == t and row[lay['tot2']][m] == t * t
                assert row[lay['alleles_subclonal']] == nas[n, s] and row[lay['subclonal']] == (nas[n, s] > 0)
                assert row[lay['loh']] == is_loh[n, s] and row[lay['hdel']] == is_hdel[n, s]
                if marg:
                    oh = row[lay['marginals']].reshape(M, 2, cmax + 1)
                    for m in range(M):
                        for a in range(2):
                            for c_ in range(cmax + 1):
                                assert oh[m, a, c_] == (dense[n, s, m, a] == c_)
    assert is_loh[1].any() and nas.max() == 2 and is_hdel.sum() == 0
    assert posteriors.feature_matrix(_classes(normals=((0, 0),)))[0][0, :, 2 * M + 3].sum() == 1      # the all-zero state, once


def test_cn_to_states_inverts_states_to_cn():
    classes = _classes()
    C, S, M, _ = classes.shape
    seg_class = np.repeat(np.arange(C), S).astype(np.int32)     # every state of every class, once
    states = np.tile(np.arange(S), C)
    cn = classes[seg_class, states]                             # states_to_cn
    assert np.array_equal(posteriors.cn_to_states(cn, classes, seg_class), states)
    stacked = np.stack([cn, cn[::-1]])                          # leading axes
    seg_rev = seg_class[::-1]
    assert np.array_equal(posteriors.cn_to_states(stacked[:1], classes, seg_class)[0], states)
    assert np.array_equal(posteriors.cn_to_states(cn[::-1], classes, seg_rev), states[::-1])
    bad = cn.copy(); bad[5, 1, 0] = classes.max() + 1
    with pytest.raises(ValueError):
        posteriors.cn_to_states(bad, classes, seg_class)
    wrong_normal = cn.copy(); wrong_normal[0, 0] = (1, 0)       # class 0 holds only the normal row (1, 1)
    with pytest.raises(ValueError):
        posteriors.cn_to_states(wrong_normal, classes, seg_class)


def _small_posterior(seed=0, N=9):
    rng = np.random.RandomState(seed)
    classes = _classes()
    seg_class = rng.randint(0, classes.shape[0], size=N).astype(np.int32)
    post = rng.dirichlet(np.full(classes.shape[1], 0.3), size=N)
    return classes, seg_class, post, rng


def test_unpack_and_stats_by_enumeration():
    classes, seg_class, post, rng = _small_posterior()
    C, S, M, _ = classes.shape
    N = len(seg_class)
    W, lay = posteriors.feature_matrix(classes, marginals=True)
    states = rng.randint(0, S, size=N)
    proj, stats, amax = twin.summary(post, W, seg_class, states)
    s = posteriors.unpack(proj, stats, amax, lay, classes, seg_class)
    cmax = int(classes.max())
    mean = np.zeros((N, M)); sq = np.zeros((N, M)); marg = np.zeros((N, M, 2, cmax + 1))
    p_sub = np.zeros(N); p_loh = np.zeros(N); p_hdel = np.zeros(N); e_sub = np.zeros(N)
    for n in range(N):
        for st in range(S):
            cn = classes[seg_class[n], st]
            p = post[n, st]
            mean[n] += p * cn.sum(axis=1); sq[n] += p * cn.sum(axis=1) ** 2
            k = int((cn[1:].max(axis=0) != cn[1:].min(axis=0)).sum())
            e_sub[n] += p * k; p_sub[n] += p * (k > 0)
            p_loh[n] += p * bool((cn.sum(axis=0) == 0).any()); p_hdel[n] += p * bool((cn == 0).all())
            for m in range(M):
                for a in range(2):
                    marg[n, m, a, cn[m, a]] += p
    tol = dict(rtol=1e-13, atol=1e-14)
    assert np.allclose(s['total_cn_mean'], mean, **tol)
    assert np.allclose(s['total_cn_sd'], np.sqrt(np.maximum(sq - mean ** 2, 0)), rtol=1e-7, atol=1e-7)
    for k, v in (('p_subclonal', p_sub), ('p_loh', p_loh), ('p_hdel', p_hdel), ('expected_alleles_subclonal', e_sub), ('cn_marginals', marg)):
        assert np.allclose(s[k], v, **tol), k
    assert np.allclose(s['cn_marginals'].sum(axis=3), 1., rtol=0, atol=1e-13)
    assert np.array_equal(s['cn_posterior_prob'], post[np.arange(N), states])
    assert np.array_equal(s['cn_posterior_max'], post.max(axis=1))
    assert np.array_equal(s['cn_mpm'], classes[seg_class, post.argmax(axis=1)])
    assert (s['cn_posterior_entropy'] > 0).all() and (s['cn_posterior_entropy'] <= np.log(S)).all()
    l = rng.uniform(1e3, 1e6, size=N)
    st = posteriors.summary_stats(s, l)
    assert np.isclose(st['ploidy_posterior_mean'], (mean[:, 1:].sum(axis=1) * l).sum() / ((M - 1) * l.sum()), rtol=1e-13)
    assert np.isclose(st['proportion_divergent_posterior_mean'], (e_sub * l).sum() / (2 * l.sum()), rtol=1e-13)
    # without a projection / statistics only those keys are left out
    assert set(posteriors.unpack(None, stats, None, lay)) == {'cn_posterior_prob', 'cn_posterior_max', 'cn_posterior_entropy'}


def test_point_mass_reproduces_the_path_statistics():
    classes, seg_class, _, rng = _small_posterior(seed=3, N=40)
    S = classes.shape[1]
    states = rng.randint(0, S, size=len(seg_class))
    post = np.zeros((len(seg_class), S)); post[np.arange(len(seg_class)), states] = 1.
    cn = classes[seg_class, states]
    l = rng.uniform(1e3, 1e6, size=len(seg_class))
    W, lay = posteriors.feature_matrix(classes)
    proj, stats, amax = twin.summary(post, W, seg_class, states)
    s = posteriors.unpack(proj, stats, amax, lay, classes, seg_class)
    st = posteriors.summary_stats(s, l)
    ploidy, divergent = tumour_ploidy_and_divergence(cn, l)
    prop = (divergent.T * l).sum() / (2. * l.sum())
    assert prop > 0
    assert abs(st['ploidy_posterior_mean'] - ploidy) <= 1e-12 * abs(ploidy)
    assert abs(st['proportion_divergent_posterior_mean'] - prop) <= 1e-12 * abs(prop)
    assert np.array_equal(s['cn_mpm'], cn) and (s['total_cn_sd'] == 0).all() and (s['cn_posterior_entropy'] == 0).all()
    assert (s['cn_posterior_prob'] == 1).all()


def test_record_round_trip_and_unchanged_when_off():
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=4, num_chains=3, seed=2)
    ps = synthetic.make_init_params(e, 3, 4)
    rng = np.random.RandomState(0)
    names = ['negbin_r_0', 'negbin_r_1', 'betabin_M_0', 'betabin_M_1']
    N, M = len(e.x), 3
    brk_ids = list(e.breakpoints.keys())
    plain = [_fake_result(e, rng) for _ in ps]
    with_post = []
    for res in plain:
        r2 = dict(res, stats=dict(res['stats']))
        summary = dict((k, rng.uniform(size=(N, M) if k.startswith('total_cn') else (N,))) for k in posteriors.COMPACT_ARRAYS)
        summary['expected_alleles_subclonal'] = rng.uniform(0, 2, size=N)
        with_post.append(posteriors.add_posterior_summary(r2, summary, e.l))
        assert set(posteriors.COMPACT_ARRAYS) <= set(r2) and set(posteriors.SUMMARY_STATS) <= set(r2['stats'])
    for a, b in zip(plain, with_post):
        fa, ia = restarts._pack(a, N, M, len(brk_ids), 4, brk_ids, names)
        fb, ib = restarts._pack(b, N, M, len(brk_ids), 4, brk_ids, names, cn_posterior=False)
        assert fa.tobytes() == fb.tobytes() and ia.tobytes() == ib.tobytes()
        assert len(fa) == restarts._HDR + M + 4 + 4 * N
        fc, _ = restarts._pack(b, N, M, len(brk_ids), 4, brk_ids, names, cn_posterior=True)
        assert len(fc) == len(fa) + N * (6 + 2 * M) + 2 and fc[:len(fa)].tobytes() == fa.tobytes()
    off = restarts.gather_result_records(with_post, e, ps, M, names)
    for i, res in off.items():
        assert not (set(posteriors.COMPACT_ARRAYS) & set(res)) and not (set(posteriors.SUMMARY_STATS) & set(res['stats']))
    on = restarts.gather_result_records(with_post, e, ps, M, names, cn_posterior=True)
    for i, res in on.items():
        src = with_post[i]
        for k in posteriors.COMPACT_ARRAYS:
            assert res[k].shape == np.shape(src[k]) and np.array_equal(res[k], src[k]), k
        for k in posteriors.SUMMARY_STATS:
            assert res['stats'][k] == src['stats'][k]
        assert np.array_equal(res['cn'], src['cn']) and res['stats']['elbo'] == src['stats']['elbo']
        assert np.array_equal(res['p_outlier_total'], off[i]['p_outlier_total'])
        assert sorted(set(res) - set(posteriors.COMPACT_ARRAYS)) == sorted(off[i])
