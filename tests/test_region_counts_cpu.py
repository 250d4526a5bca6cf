"""Host side of the region change counts (remixt_amd/posteriors.py) and their numpy twin, without a GPU: the twin against
brute-force path enumeration, the convolution of a split region's pieces, the distributed record with and without
config cn_region_change_bins, and the config checks."""
import itertools

import numpy as np
import pytest

from remixt_amd import defaults, posteriors, restarts, synthetic
from tests import region_counts_twin, region_twin
from tests.test_cn_samples_records_cpu import _fake_result


def test_twin_against_enumeration():
    rng = np.random.RandomState(11)
    N, S = 6, 3
    f = rng.normal(scale=2., size=(N, S))
    T = rng.normal(scale=2., size=(N - 1, S, S))
    twin = region_counts_twin.CountsTwin(f, T, [0], [N - 1])
    mask = rng.uniform(size=(N, S)) < 0.6
    mask[np.arange(N), rng.randint(0, S, size=N)] = True
    label = rng.randint(0, 2, size=(N, S))
    identity = np.tile(np.arange(S), (N, 1))
    holes = np.array([1, 0, 1, 1, 0, 1], dtype=bool)
    cases = [dict(label=label), dict(label=identity), dict(label=label, mask=mask), dict(label=identity, mask=mask, constrain=holes)]
    runs = list(itertools.combinations_with_replacement(range(N), 2))
    assert (0, 3) in runs and (2, N - 1) in runs and (0, N - 1) in runs      # from the chain start, to the chain end, both
    saturated = 0
    for a, b in runs:
        for kw in cases:
            for K in (1, 2, 4):
                want = region_counts_twin.brute_force_counts(f, T, a, b, K, **kw)
                got = twin.logcounts(a, b, K, **kw)
                assert got.shape == (K,)
                assert np.array_equal(got == -np.inf, want == -np.inf), (a, b, K, sorted(kw), got, want)
                assert (np.abs(np.exp(got) - np.exp(want)) <= 1e-12).all(), (a, b, K, sorted(kw), got, want)
                saturated += b - a > K - 1 and want[K - 1] > -np.inf
                if K > 1:
                    assert (got[b - a + 1:] == -np.inf).all()      # more changes than adjacencies
            # the bins add up to the event without the count, and bin 0 is the event "no change"
            kw0 = dict((k, v) for k, v in kw.items() if k != 'label')
            full = twin.logcounts(a, b, 4, **kw)
            assert abs(np.exp(full).sum() - np.exp(twin.logprob(a, b, **kw0))) <= 1e-12
            assert abs(np.exp(full[0]) - np.exp(twin.logprob(a, b, **kw))) <= 1e-12
            assert abs(np.exp(twin.logcounts(a, b, 1, **kw)[0]) - np.exp(twin.logprob(a, b, **kw0))) <= 1e-12
    assert saturated >= 20


def test_twin_with_two_chains():
    rng = np.random.RandomState(6)
    S = 3
    f = rng.normal(size=(7, S)); T = rng.normal(size=(6, S, S))
    T[3] = 0.      # (the adjacency across the chain end, as log_transmat holds it)
    both = region_counts_twin.CountsTwin(f, T, [0, 4], [3, 6])
    label = rng.randint(0, 2, size=(7, S))
    assert np.abs(np.exp(both.logcounts(1, 3, 3, label)) - np.exp(region_counts_twin.brute_force_counts(f[:4], T[:3], 1, 3, 3, label[:4]))).max() <= 1e-12
    assert np.abs(np.exp(both.logcounts(4, 6, 3, label)) - np.exp(region_counts_twin.brute_force_counts(f[4:], T[4:], 0, 2, 3, label[4:]))).max() <= 1e-12


def _convolve(ps, K):
    """Distribution of the sum of independent counts with distributions ps (last bin: K - 1 or more), by enumeration."""
    out = np.zeros(K)
    for ks in itertools.product(range(K), repeat=len(ps)):
        out[min(sum(ks), K - 1)] += np.prod([p[k] for p, k in zip(ps, ks)])
    return out


def test_combine_counts():
    rng = np.random.RandomState(3)
    K = 4
    p = rng.dirichlet(np.ones(K), size=6)
    p[1] = [0.25, 0., 0.75, 0.]              # bins that cannot happen: -inf
    p[4] = [0., 0., 0., 1.]                  # all of it in the saturating bin
    piece_region = np.array([0, 0, 1, 2, 2, 2])
    with np.errstate(divide='ignore'):
        logp = np.log(p)
    assert (logp[1] == -np.inf).sum() == 2
    got = posteriors.combine_counts(logp, piece_region, 4)
    assert got.shape == (4, K)
    assert np.abs(got[0] - _convolve([p[0], p[1]], K)).max() <= 1e-15
    assert np.array_equal(got[1], p[2])                                  # one piece: its own distribution
    assert np.abs(got[2] - _convolve([p[3], p[4], p[5]], K)).max() <= 1e-15
    assert np.abs(got[2] - [0, 0, 0, 1]).max() <= 1e-15                  # a saturated piece saturates the region
    assert np.array_equal(got[3], [1, 0, 0, 0])                          # no piece: no change
    assert np.abs(got.sum(axis=1) - 1).max() <= 1e-15
    # leading axes (restarts), and one bin
    two = posteriors.combine_counts(np.stack([logp, logp[::-1]]), piece_region, 3)
    assert two.shape == (2, 3, K) and np.array_equal(two[0], got[:3])
    assert np.abs(two[1, 0] - _convolve([p[5], p[4]], K)).max() <= 1e-15
    one = posteriors.combine_counts(np.log([[0.5], [0.5], [0.25]]), [0, 0, 1], 2)
    assert np.allclose(one[:, 0], [0.25, 0.25], rtol=1e-15)


def test_record_round_trip_and_unchanged_when_off():
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=4, num_chains=3, seed=2)
    ps = synthetic.make_init_params(e, 3, 4)
    rng = np.random.RandomState(0)
    names = ['negbin_r_0', 'negbin_r_1', 'betabin_M_0', 'betabin_M_1']
    N, M, K = len(e.x), 3, 5
    brk_ids = list(e.breakpoints.keys())
    region_names = ['geneA', 'arm', 'one']
    plain = [_fake_result(e, rng) for _ in ps]
    with_counts = []
    for res in plain:
        r2 = dict(res, stats=dict(res['stats']))
        posteriors.add_region_events(r2, region_names, dict((k, rng.uniform(size=3)) for k in posteriors.REGION_ARRAYS))
        posteriors.add_region_change_counts(r2, region_names, K, dict((k, rng.dirichlet(np.ones(K), size=3)) for k in posteriors.COUNT_ARRAYS))
        assert sorted(r2['region_change_counts']) == ['bins', 'names', 'num_changes', 'num_total_changes']
        with_counts.append(r2)
    for a, b in zip(plain, with_counts):
        fa, ia = restarts._pack(a, N, M, len(brk_ids), 4, brk_ids, names)
        assert len(fa) == restarts._HDR + M + 4 + 4 * N
        # off: slot counts unchanged, with and without regions
        fb, ib = restarts._pack(b, N, M, len(brk_ids), 4, brk_ids, names, region_names=None, change_bins=K)
        assert fa.tobytes() == fb.tobytes() and ia.tobytes() == ib.tobytes()
        fr, ir = restarts._pack(b, N, M, len(brk_ids), 4, brk_ids, names, region_names=region_names)
        fr0, _ = restarts._pack(b, N, M, len(brk_ids), 4, brk_ids, names, region_names=region_names, change_bins=0)
        assert len(fr) == len(fa) + 7 * 3 and fr.tobytes() == fr0.tobytes()
        # on: 2 K slots per region, after everything else
        fc, ic = restarts._pack(b, N, M, len(brk_ids), 4, brk_ids, names, region_names=region_names, change_bins=K)
        assert len(fc) == len(fr) + 2 * K * 3 and fc[:len(fr)].tobytes() == fr.tobytes() and ic.tobytes() == ir.tobytes()
    off = restarts.gather_result_records(with_counts, e, ps, M, names, region_names=region_names)
    on = restarts.gather_result_records(with_counts, e, ps, M, names, region_names=region_names, change_bins=K)
    for i, res in on.items():
        assert 'region_change_counts' not in off[i] and sorted(set(res) - {'region_change_counts'}) == sorted(off[i])
        src, got = with_counts[i]['region_change_counts'], res['region_change_counts']
        assert got['names'] == region_names and got['bins'] == K
        for k in posteriors.COUNT_ARRAYS:
            assert got[k].shape == (3, K) and np.array_equal(got[k], src[k]), k
        for k in posteriors.REGION_ARRAYS:
            assert np.array_equal(res['region_events'][k], with_counts[i]['region_events'][k]), k
        assert np.array_equal(res['cn'], with_counts[i]['cn']) and res['stats']['elbo'] == with_counts[i]['stats']['elbo']
    # next to the posterior summary block
    full = []
    for res in with_counts:
        r3 = dict(res, stats=dict(res['stats']))
        summary = dict((k, rng.uniform(size=(N, M) if k.startswith('total_cn') else (N,))) for k in posteriors.COMPACT_ARRAYS)
        summary['expected_alleles_subclonal'] = rng.uniform(0, 2, size=N)
        posteriors.add_posterior_summary(r3, summary, e.l)
        full.append(r3)
    both = restarts.gather_result_records(full, e, ps, M, names, cn_posterior=True, region_names=region_names, change_bins=K)
    for i, res in both.items():
        for k in posteriors.COMPACT_ARRAYS:
            assert np.array_equal(res[k], full[i][k]), k
        for k in posteriors.REGION_ARRAYS:
            assert np.array_equal(res['region_events'][k], full[i]['region_events'][k]), k
        for k in posteriors.COUNT_ARRAYS:
            assert np.array_equal(res['region_change_counts'][k], full[i]['region_change_counts'][k]), k


def test_config():
    assert defaults.cn_region_change_bins == 0 and defaults.get_param({}, 'cn_region_change_bins') == 0
    assert posteriors.change_bins({}) == 0 and posteriors.change_bins({'cn_regions': [('a', 0, 1)]}) == 0
    assert posteriors.change_bins({'cn_regions': [('a', 0, 1)], 'cn_region_change_bins': 6}) == 6
    with pytest.raises(ValueError, match='needs cn_regions'):
        posteriors.change_bins({'cn_region_change_bins': 6})
    for bad in (17, -1):
        with pytest.raises(ValueError, match='0 .. 16'):
            posteriors.change_bins({'cn_regions': [('a', 0, 1)], 'cn_region_change_bins': bad})
    # the entry points refuse it before any fit
    from remixt_amd.analysis import pipeline
    e = synthetic.make_experiment(20, num_clones=3, max_copy_number=3, num_chains=2, seed=0)
    ps = synthetic.make_init_params(e, 2, 3)
    with pytest.raises(ValueError, match='needs cn_regions'):
        pipeline.fit_restarts(e, dict(enumerate(ps)), {'cn_region_change_bins': 4})
    with pytest.raises(ValueError, match='needs cn_regions'):
        pipeline.fit(e, ps[0], {'cn_region_change_bins': 4})
    with pytest.raises(ValueError, match='needs cn_regions'):
        restarts.fit_restarts_distributed(e, ps, 3, cn_region_change_bins=4)
    assert region_twin.LD is np.longdouble
