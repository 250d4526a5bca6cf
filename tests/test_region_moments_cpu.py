"""Host side of the region moments (remixt_amd/posteriors.py) and their numpy twin, without a GPU: the twin against
brute-force path enumeration, combine_moments / batch_region_cn_moments / moment_stats against a batch answered by the
twin, the distributed record with and without cn_moments, the config check, the declarations."""
import itertools

import numpy as np
import pytest

from remixt_amd import defaults, posteriors, restarts, synthetic
from tests import region_moments_twin, region_twin
from tests.test_cn_samples_records_cpu import _fake_result


def _unpack(flat, nf):
    return posteriors._moment_matrices(flat, nf)


def test_twin_against_enumeration():
    rng = np.random.RandomState(11)
    N, S, nf = 6, 4, 3
    f = rng.normal(scale=2., size=(N, S))
    T = rng.normal(scale=2., size=(N - 1, S, S))
    twin = region_moments_twin.MomentsTwin(region_twin.RegionTwin(f, T, [0], [N - 1]))
    feat = rng.normal(size=(N, nf, S))
    feat[:, 1] = rng.randint(0, 2, size=(N, S))          # an indicator
    feat[2, 0] = 1.5                                     # constant at one segment ("in a class"): no variance from it there
    w = rng.uniform(0.5, 3., size=N)
    w[3] = 0.                                            # a zero weight inside the runs
    worst_m = worst_c = 0.
    for a, b in itertools.combinations_with_replacement(range(N), 2):
        wm, wc = region_moments_twin.brute_force(f, T, a, b, feat, w)
        gm, gc = twin.moments(a, b, feat, w)
        B = np.array([sum(abs(w[n]) * np.abs(feat[n, k]).max() for n in range(a, b + 1)) for k in range(nf)])
        worst_m = max(worst_m, (np.abs(gm - wm) / np.maximum(B, 1e-300)).max())
        worst_c = max(worst_c, (np.abs(gc - wc) / np.maximum(np.outer(B, B), 1e-300)).max())
        assert (np.abs(gm - wm) <= 1e-12 * B).all(), (a, b, gm, wm)
        assert (np.abs(gc - wc) <= 1e-12 * np.outer(B, B)).all(), (a, b, gc, wc)
        assert np.array_equal(gc, gc.T)
        if a == b == 2:
            assert abs(gc[0, 0]) <= 1e-15 and np.abs(gc[0]).max() <= 1e-15      # the constant feature
        if a == b == 3:
            assert np.abs(gc).max() == 0 and np.abs(gm).max() == 0              # the zero weight
    print('twin against enumeration: worst |mean| / B %.3e, worst |cov| / B^2 %.3e' % (worst_m, worst_c))


def test_twin_signed_feature_and_two_chains():
    rng = np.random.RandomState(6)
    S = 3
    f = rng.normal(size=(7, S)); T = rng.normal(size=(6, S, S))
    T[3] = 0.      # (the adjacency across the chain end, as log_transmat holds it)
    both = region_moments_twin.MomentsTwin(region_twin.RegionTwin(f, T, [0, 4], [3, 6]))
    phi = rng.normal(size=(7, 1, S))
    feat = np.concatenate([phi, -phi], axis=1)           # F_1 = -F_0: Cov(F_0, F_1) = -Var(F_0) < 0
    w = rng.uniform(0.5, 2., size=7); w[5] = 0.
    for (a, b), (lo, hi) in (((1, 3), (0, 4)), ((4, 6), (4, 7)), ((0, 3), (0, 4))):
        gm, gc = both.moments(a, b, feat, w)
        wm, wc = region_moments_twin.brute_force(f[lo:hi], T[lo:hi - 1], a - lo, b - lo, feat[lo:hi], w[lo:hi])
        assert np.abs(gm - wm).max() <= 1e-12 and np.abs(gc - wc).max() <= 1e-12
        assert gc[0, 0] > 1e-3 and gc[0, 1] < 0 and abs(gc[0, 1] + gc[0, 0]) <= 1e-12 and abs(gm[0] + gm[1]) <= 1e-12


class TwinBatch(object):
    """What posteriors.batch_region_cn_moments needs of a RemixtBatch, answered by the twin: one dense (framelogprob,
    log_transmat) per restart."""

    def __init__(self, cn_classes, seg_class, framelogprobs, log_transmats, chain_start, chain_end):
        self.cn_classes = np.asarray(cn_classes)
        self.seg_class = np.asarray(seg_class)
        self.num_segments, self.num_cn_states = np.asarray(framelogprobs[0]).shape
        self.rtwins = [region_twin.RegionTwin(f, T, chain_start, chain_end) for f, T in zip(framelogprobs, log_transmats)]
        self.twins = [region_moments_twin.MomentsTwin(t) for t in self.rtwins]
        self.calls = []      # (nr, nq, nf) of every call

    def region_moments_raw(self, r0, nr, queries, features, weights, nf):
        queries, features, weights = np.asarray(queries).reshape(-1, 4), np.asarray(features), np.asarray(weights)
        self.calls.append((nr, len(queries), nf))
        out = np.zeros((nr, len(queries), nf + nf * (nf + 1) // 2))
        iu = np.triu_indices(nf)
        for i in range(nr):
            for j, (a, b, f0, wi) in enumerate(queries):
                mean, cov = self.twins[r0 + i].moments(a, b, features[self.seg_class][:, f0:f0 + nf], weights[wi])
                out[i, j, :nf], out[i, j, nf:] = mean, cov[iu]
        return out


def _twin_batch(nr=2, seed=3, M=2):
    """Seven experiment segments in two chains; the model inserts zero-length segments at 2 and 6 (nine model segments)."""
    rng = np.random.RandomState(seed)
    S = 6
    cn_classes = np.zeros((1, S, M, 2), dtype=int)
    cn_classes[0, :, 0] = (1, 1)
    cn_classes[0, :, 1] = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2)]
    for m in range(2, M):
        cn_classes[0, :, m] = cn_classes[0, rng.permutation(S), 1]
    N1 = 9
    tel = np.array([0, 0, 0, 0, 1, 0, 0, 0, 0])
    fs = [rng.normal(scale=1.5, size=(N1, S)) for _ in range(nr)]
    Ts = []
    for _ in range(nr):
        T = rng.normal(scale=1.5, size=(N1 - 1, S, S))
        T[4] = 0.
        Ts.append(T)
    cs, ce = posteriors.chains_from_telomeres(tel)
    b = TwinBatch(cn_classes, np.zeros(N1, dtype=int), fs, Ts, cs, ce)
    fwd = np.array([0, 1, 3, 4, 5, 7, 8])
    orig = np.ones(N1, dtype=bool); orig[[2, 6]] = False
    l1 = rng.uniform(1e3, 1e5, size=N1) * orig
    return b, fwd, orig, tel, l1


def test_moment_features():
    b, _, _, _, _ = _twin_batch(M=3)
    W, layout = posteriors.feature_matrix(b.cn_classes)
    F = posteriors.moment_features(b.cn_classes)
    assert F.shape == (1, 3 + 4, 6) and F.dtype == np.float64 and F.flags['C_CONTIGUOUS']
    assert np.array_equal(F[:, :3], W[:, :, layout['tot']].transpose(0, 2, 1))
    assert posteriors.MOMENT_FRACTIONS == ('alleles_subclonal', 'subclonal', 'loh', 'hdel')
    for i, k in enumerate(posteriors.MOMENT_FRACTIONS):
        assert np.array_equal(F[:, 3 + i], W[:, :, layout[k]]), k


def test_combine_moments():
    rng = np.random.RandomState(3)
    out = rng.normal(size=(2, 6, 5))
    piece_region = np.array([0, 0, 1, 2, 2, 2])
    got = posteriors.combine_moments(out, piece_region, 4)
    assert got.shape == (2, 4, 5)
    assert np.allclose(got[:, 0], out[:, 0] + out[:, 1], rtol=1e-15) and np.array_equal(got[:, 1], out[:, 2])
    assert np.allclose(got[:, 2], out[:, 3] + out[:, 4] + out[:, 5], rtol=1e-15) and (got[:, 3] == 0).all()
    # independence: the covariance of a sum over two independent chains by enumeration of the product
    b, _, _, _, _ = _twin_batch(nr=1)
    feat = rng.normal(size=(9, 2, 6)); w = rng.uniform(1, 2, size=9)
    t = b.rtwins[0]
    m1, c1 = region_moments_twin.brute_force(t.f[:5], np.log(t.E[:4]), 0, 4, feat[:5], w[:5])
    m2, c2 = region_moments_twin.brute_force(t.f[5:], np.log(t.E[5:]), 1, 3, feat[5:], w[5:])
    iu = np.triu_indices(2)
    flat = np.array([np.concatenate([m1, c1[iu]]), np.concatenate([m2, c2[iu]])])
    mean, cov = _unpack(posteriors.combine_moments(flat, [0, 0], 1), 2)
    g1, h1 = b.twins[0].moments(0, 4, feat, w)
    g2, h2 = b.twins[0].moments(6, 8, feat, w)
    assert np.abs(mean[0] - (g1 + g2)).max() <= 1e-12 and np.abs(cov[0] - (h1 + h2)).max() <= 1e-12
    assert np.array_equal(cov[0], cov[0].T)


@pytest.mark.parametrize('M', [2, 4])
def test_batch_region_cn_moments(M):
    b, fwd, orig, tel, l1 = _twin_batch(M=M)
    # across the chain end, holding the inserted segment 2, a single segment, holding the inserted segment 6, the whole genome
    regions = [(0, 6), (1, 2), (3, 3), (4, 5), (0, 6)]
    pieces = [[(0, 4), (5, 8)], [(1, 3)], [(4, 4)], [(5, 7)], [(0, 4), (5, 8)]]
    out = posteriors.batch_region_cn_moments(b, 0, 2, regions, fwd, orig, tel, l1)
    P = sum(len(p) for p in pieces)
    # one device call when both groups have four features, one per group otherwise
    assert b.calls == ([(2, 2 * P, 4)] if M == 4 else [(2, P, M), (2, P, 4)])
    assert sorted(out) == sorted(posteriors.MOMENT_ARRAYS)
    shapes = posteriors.moment_shapes(len(regions), M)
    assert out['length'].shape == shapes['length'] and all(out[k].shape == (2,) + shapes[k] for k in posteriors.MOMENT_ARRAYS[1:])
    F = posteriors.moment_features(b.cn_classes)[b.seg_class]       # (N1, M + 4, S)
    for r in range(2):
        for j, runs in enumerate(pieces):
            L = sum(l1[a:e + 1].sum() for a, e in runs)
            assert abs(out['length'][j] - L) <= 1e-9 * L
            for name, sl in (('total_cn', slice(0, M)), ('fraction', slice(M, M + 4))):
                mean = sum(b.twins[r].moments(a, e, F[:, sl], l1)[0] for a, e in runs) / L
                cov = sum(b.twins[r].moments(a, e, F[:, sl], l1)[1] for a, e in runs) / L ** 2
                assert np.abs(out[name + '_mean'][r, j] - mean).max() <= 1e-12 * np.abs(F[:, sl]).max(), (name, r, j)
                assert np.abs(out[name + '_cov'][r, j] - cov).max() <= 1e-12 * np.abs(F[:, sl]).max() ** 2, (name, r, j)
                assert np.array_equal(out[name + '_cov'][r, j], out[name + '_cov'][r, j].T)
    # fractions of indicators lie in [0, 1]; the variance of a single segment's indicator is p (1 - p)
    assert ((out['fraction_mean'][..., 1:] >= 0) & (out['fraction_mean'][..., 1:] <= 1)).all()
    p = out['fraction_mean'][:, 2, 2]
    assert np.abs(out['fraction_cov'][:, 2, 2, 2] - p * (1 - p)).max() <= 1e-12
    # the whole-genome ploidy mean is summary_stats' (the per-segment means of the marginals, experiment order)
    for r in range(2):
        marg = b.twins[r].marg.astype(float)
        summary = {'total_cn_mean': (marg @ F[0, :M].T)[fwd], 'expected_alleles_subclonal': (marg @ F[0, M])[fwd]}
        want = posteriors.summary_stats(summary, l1[fwd])
        got = out['total_cn_mean'][r, 4, 1:].sum() / (M - 1)
        assert abs(got - want['ploidy_posterior_mean']) <= 1e-12 * abs(want['ploidy_posterior_mean'])
        assert abs(out['fraction_mean'][r, 4, 0] / 2 - want['proportion_divergent_posterior_mean']) <= 1e-12
        sd = posteriors.moment_stats(*[out[k][r, 4] for k in posteriors.MOMENT_ARRAYS[1:]])
        assert sorted(sd) == sorted(posteriors.MOMENT_STATS)
        ones = np.ones(M - 1)
        assert abs(sd['ploidy_posterior_sd'] - np.sqrt(ones @ out['total_cn_cov'][r, 4][1:, 1:] @ ones) / (M - 1)) <= 1e-15
        assert abs(sd['proportion_divergent_posterior_sd'] - np.sqrt(out['fraction_cov'][r, 4, 0, 0]) / 2) <= 1e-15
        # (one tumour clone has no subclonal alleles: that SD is exactly 0)
        assert sd['ploidy_posterior_sd'] > 0 and (sd['proportion_divergent_posterior_sd'] > 0) == (M > 2)
    # a region of length 0 (only possible with zero-length segments): NaN, the others unchanged
    l0 = l1.copy(); l0[4] = 0.
    z = posteriors.batch_region_cn_moments(b, 0, 2, regions, fwd, orig, tel, l0)
    assert z['length'][2] == 0 and all(np.isnan(z[k][:, 2]).all() for k in posteriors.MOMENT_ARRAYS[1:])
    assert all(np.isfinite(z[k][:, [0, 1, 3, 4]]).all() for k in posteriors.MOMENT_ARRAYS[1:])
    # restart range, and no regions: no device call
    one = posteriors.batch_region_cn_moments(b, 1, 1, regions, fwd, orig, tel, l1)
    assert all(np.array_equal(one[k][0], out[k][1]) for k in posteriors.MOMENT_ARRAYS[1:])
    ncalls = len(b.calls)
    empty = posteriors.batch_region_cn_moments(b, 0, 2, [], fwd, orig, tel, l1)
    assert empty['length'].shape == (0,) and empty['total_cn_cov'].shape == (2, 0, M, M) and len(b.calls) == ncalls
    # the appended whole-genome region
    assert posteriors.genome_region([(1, 2)], 7).tolist() == [[1, 2], [0, 6]] and posteriors.genome_region([], 7).tolist() == [[0, 6]]


def _fake_moments(rng, R, M):
    shapes = posteriors.moment_shapes(R, M)
    return dict((k, rng.uniform(size=shapes[k])) for k in posteriors.MOMENT_ARRAYS)


def test_record_round_trip_and_unchanged_when_off():
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=4, num_chains=3, seed=2)
    ps = synthetic.make_init_params(e, 3, 4)
    rng = np.random.RandomState(0)
    names = ['negbin_r_0', 'negbin_r_1', 'betabin_M_0', 'betabin_M_1']
    N, M, K = len(e.x), 3, 5
    brk_ids = list(e.breakpoints.keys())
    region_names = ['geneA', 'arm', 'one']
    R = len(region_names)
    per_region = 1 + M + M * M + 4 + 16
    full = []
    for _ in ps:
        r2 = _fake_result(e, rng)
        posteriors.add_region_events(r2, region_names, dict((k, rng.uniform(size=R)) for k in posteriors.REGION_ARRAYS))
        posteriors.add_region_change_counts(r2, region_names, K, dict((k, rng.dirichlet(np.ones(K), size=R)) for k in posteriors.COUNT_ARRAYS))
        posteriors.add_call_confidence(r2, region_names, dict((k, rng.uniform(size=R)) for k in posteriors.CALL_ARRAYS), -rng.uniform(1, 50))
        # the named regions, then the whole genome: the stats come from the last entry, which is not kept
        mom = _fake_moments(rng, R + 1, M)
        posteriors.add_region_cn_moments(r2, region_names, mom)
        got = r2['region_cn_moments']
        assert sorted(got) == sorted(('names',) + posteriors.MOMENT_ARRAYS) and all(len(got[k]) == R for k in posteriors.MOMENT_ARRAYS)
        want = posteriors.moment_stats(*[mom[k][R] for k in posteriors.MOMENT_ARRAYS[1:]])
        assert all(r2['stats'][k] == want[k] for k in posteriors.MOMENT_STATS)
        full.append(r2)
    for b in full:
        nb = len(brk_ids)
        # off: the vectors of a call that omits the keyword, with every combination of the other sections
        for kw in (dict(), dict(region_names=region_names), dict(region_names=region_names, change_bins=K),
                   dict(region_names=region_names, change_bins=K, call_confidence=True), dict(region_names=region_names, call_confidence=True)):
            f0, i0 = restarts._pack(b, N, M, nb, 4, brk_ids, names, **kw)
            f1, i1 = restarts._pack(b, N, M, nb, 4, brk_ids, names, cn_moments=False, **kw)
            assert f0.tobytes() == f1.tobytes() and i0.tobytes() == i1.tobytes()
            if 'region_names' not in kw:       # without regions the option adds nothing
                f2, i2 = restarts._pack(b, N, M, nb, 4, brk_ids, names, cn_moments=True)
                assert f0.tobytes() == f2.tobytes() and i0.tobytes() == i2.tobytes()
                continue
            # on: the section after everything else, the two stats last
            f2, i2 = restarts._pack(b, N, M, nb, 4, brk_ids, names, cn_moments=True, **kw)
            assert len(f2) == len(f0) + R * per_region + 2 and f2[:len(f0)].tobytes() == f0.tobytes() and i2.tobytes() == i0.tobytes()
            assert f2[-2] == b['stats']['ploidy_posterior_sd'] and f2[-1] == b['stats']['proportion_divergent_posterior_sd']
            assert np.array_equal(f2[len(f0):len(f0) + R], b['region_cn_moments']['length'])
            assert np.array_equal(f2[-2 - 16 * R:-2], b['region_cn_moments']['fraction_cov'].ravel())
    off = restarts.gather_result_records(full, e, ps, M, names, region_names=region_names, change_bins=K, call_confidence=True)
    on = restarts.gather_result_records(full, e, ps, M, names, region_names=region_names, change_bins=K, call_confidence=True, cn_moments=True)
    only = restarts.gather_result_records(full, e, ps, M, names, region_names=region_names, cn_moments=True)
    for i, res in on.items():
        assert 'region_cn_moments' not in off[i] and not any(k in off[i]['stats'] for k in posteriors.MOMENT_STATS)
        assert sorted(set(res) - {'region_cn_moments'}) == sorted(off[i])
        assert sorted(set(res['stats']) - set(posteriors.MOMENT_STATS)) == sorted(off[i]['stats'])
        for got in (res, only[i]):
            assert got['region_cn_moments']['names'] == region_names
            for k in posteriors.MOMENT_ARRAYS:
                assert got['region_cn_moments'][k].shape == posteriors.moment_shapes(R, M)[k]
                assert np.array_equal(got['region_cn_moments'][k], full[i]['region_cn_moments'][k]), k
            for k in posteriors.MOMENT_STATS:
                assert got['stats'][k] == full[i]['stats'][k]
        for k in posteriors.CALL_ARRAYS:
            assert np.array_equal(res['call_confidence'][k], full[i]['call_confidence'][k]), k
        for k in posteriors.COUNT_ARRAYS:
            assert np.array_equal(res['region_change_counts'][k], full[i]['region_change_counts'][k]), k
        assert res['stats']['cn_logprob'] == full[i]['stats']['cn_logprob'] and 'call_confidence' not in only[i]


def test_config():
    assert defaults.cn_region_moments is False and defaults.get_param({}, 'cn_region_moments') is False
    assert posteriors.region_moments_on({}) is False and posteriors.region_moments_on({'cn_regions': [('a', 0, 1)]}) is False
    assert posteriors.region_moments_on({'cn_regions': [('a', 0, 1)], 'cn_region_moments': True}) is True
    with pytest.raises(ValueError, match='cn_region_moments needs cn_regions'):
        posteriors.region_moments_on({'cn_region_moments': True})
    posteriors.check_region_options(None, 0, False)      # (the earlier three-argument form)
    # the entry points refuse it before any fit
    from remixt_amd.analysis import pipeline
    e = synthetic.make_experiment(20, num_clones=3, max_copy_number=3, num_chains=2, seed=0)
    ps = synthetic.make_init_params(e, 2, 3)
    with pytest.raises(ValueError, match='cn_region_moments needs cn_regions'):
        pipeline.fit_restarts(e, dict(enumerate(ps)), {'cn_region_moments': True})
    with pytest.raises(ValueError, match='cn_region_moments needs cn_regions'):
        pipeline.fit(e, ps[0], {'cn_region_moments': True})
    with pytest.raises(ValueError, match='cn_region_moments needs cn_regions'):
        restarts.fit_restarts_distributed(e, ps, 3, cn_region_moments=True)


def test_oracle_module_has_no_region_moments():
    from oracle import oracle
    from tests import helpers as H
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError):
        mo.region_cn_moments([(0, 3)])
    with pytest.raises(NotImplementedError):
        mo.ploidy_posterior_sd()


def test_declared_and_bound():
    import os
    from remixt_amd import _lib
    assert 'rmx_region_moments' in _lib.SYMBOLS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'remixt_amd.h')) as fh:
        assert 'int rmx_region_moments(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries' in fh.read()
