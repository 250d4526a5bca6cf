"""Posterior path sampling, host side: the CPU twin of the device sampler, its generator, the sample summaries."""
import itertools

import numpy as np

from remixt_amd import sampling
from remixt_amd.restarts import tumour_ploidy_and_divergence
from tests import ffbs_twin


def test_philox_known_answers():
    # Random123 known-answer vectors for philox4x32-10
    assert ffbs_twin.philox4x32_10_scalar([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert ffbs_twin.philox4x32_10_scalar([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert ffbs_twin.philox4x32_10_scalar([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_uniform_vectorised_equals_scalar():
    rng = np.random.RandomState(3)
    for seed in [0, 1, 2 ** 64 - 1, int(rng.randint(0, 2 ** 62)), sampling.restart_seed(7, 3)]:
        ks = np.array([0, 1, 5, 63, 4095, 2 ** 31 - 1])
        for n in [0, 1, 17, 49999]:
            v = ffbs_twin.uniform53(seed, ks, n)
            s = np.array([ffbs_twin.uniform53_scalar(seed, int(k), n) for k in ks])
            assert np.array_equal(v, s)
            assert (v >= 0).all() and (v < 1).all()


def test_restart_seed_distinct():
    seeds = [sampling.restart_seed(s, i) for s in range(4) for i in range(64)]
    assert len(set(seeds)) == len(seeds) and all(0 <= x < 2 ** 64 for x in seeds)
    assert sampling.restart_seed(5, 2) == sampling.restart_seed(5, 2)


def _exact_path_probs(f, T):
    N, S = f.shape
    paths = np.array(list(itertools.product(range(S), repeat=N)))
    lp = np.array([ffbs_twin.path_logprob(f, T, p) for p in paths])
    p = np.exp(lp - lp.max())
    return paths, p / p.sum()


def test_twin_matches_exact_enumeration():
    rng = np.random.RandomState(11)
    N, S, K = 5, 3, 200000
    f = rng.normal(size=(N, S)) * 1.5
    T = rng.normal(size=(N - 1, S, S))
    T[2] = 0.      # a telomere: log_transmat 0
    paths, p = _exact_path_probs(f, T)
    states, flag = ffbs_twin.sample(f, T, seed=12345, samples=np.arange(K))
    assert not flag.any()
    code = (states * S ** np.arange(N - 1, -1, -1)).sum(axis=1)
    freq = np.bincount(code, minlength=S ** N) / K
    pcode = (paths * S ** np.arange(N - 1, -1, -1)).sum(axis=1)
    pp = np.zeros(S ** N); pp[pcode] = p
    tol = 6 * np.sqrt(pp * (1 - pp) / K) + 2. / K
    assert (np.abs(freq - pp) <= tol).all(), np.abs(freq - pp).max()


def test_summary_statistics():
    rng = np.random.RandomState(5)
    K, N, M = 7, 9, 3
    samples = rng.randint(0, 4, size=(K, N, M, 2))
    cn = samples[0].copy()
    l = rng.uniform(1, 10, size=N)
    arrays, stats = sampling.sample_summary(samples, cn, l)
    exp_agree = np.array([[np.mean([np.array_equal(samples[k, n, m], cn[n, m]) for k in range(K)]) for m in range(M)] for n in range(N)])
    exp_state = np.array([np.mean([np.array_equal(samples[k, n], cn[n]) for k in range(K)]) for n in range(N)])
    assert np.array_equal(arrays['cn_sample_agreement'], exp_agree)
    assert np.array_equal(arrays['cn_state_agreement'], exp_state)
    ploidy, prop = [], []
    for k in range(K):
        pl, div = tumour_ploidy_and_divergence(samples[k], l)
        ploidy.append(pl); prop.append((div.T * l).sum() / (2. * l.sum()))
    vp, vd = sampling.ploidy_and_divergence_samples(samples, l)
    assert np.allclose(vp, ploidy, rtol=1e-12, atol=0) and np.allclose(vd, prop, rtol=1e-12, atol=0)
    for name, v in (('ploidy', ploidy), ('proportion_divergent', prop)):
        q = np.quantile(v, [0.05, 0.5, 0.95])
        assert np.allclose([stats[name + '_q05'], stats[name + '_q50'], stats[name + '_q95']], q, rtol=1e-12, atol=0)
        assert stats[name + '_q05'] <= stats[name + '_q50'] <= stats[name + '_q95']
