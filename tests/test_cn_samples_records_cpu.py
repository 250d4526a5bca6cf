"""The distributed result record with posterior-sample summaries (config num_cn_samples > 0): round trip of the new fields, and
the record unchanged -- byte for byte -- when the option is off."""
import numpy as np

from remixt_amd import restarts, sampling, synthetic


def _fake_result(e, rng, M=3):
    N = len(e.x)
    res = {'h': rng.uniform(0.01, 1, size=M), 'cn': rng.randint(0, 5, size=(N, M, 2)),
           'brk_cn': dict((k, rng.randint(0, 3, size=M)) for k in e.breakpoints),
           'p_outlier_total': rng.uniform(size=(N, 2)), 'p_outlier_allele': rng.uniform(size=(N, 2)),
           'total_likelihood_mask': rng.randint(0, 2, size=N), 'allele_likelihood_mask': rng.randint(0, 2, size=N)}
    res['stats'] = {'elbo': -1234.5, 'elbo_diff': 0.25, 'ploidy': 2.7, 'proportion_divergent': 0.1, 'error_message': '',
                    'negbin_r_0': 1., 'negbin_r_1': 2., 'betabin_M_0': 3., 'betabin_M_1': 4.}
    return res


def test_record_round_trip_and_unchanged_when_off():
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=4, num_chains=3, seed=2)
    ps = synthetic.make_init_params(e, 3, 4)
    rng = np.random.RandomState(0)
    names = ['negbin_r_0', 'negbin_r_1', 'betabin_M_0', 'betabin_M_1']
    N, M = len(e.x), 3
    brk_ids = list(e.breakpoints.keys())
    plain = [_fake_result(e, rng) for _ in ps]
    with_smp = []
    for res in plain:
        r2 = dict(res, stats=dict(res['stats']))
        samples = rng.randint(0, 5, size=(6, N, M, 2))
        samples[:3] = res['cn']
        with_smp.append(sampling.add_sample_summary(r2, samples, e.l))
    # off: a result that carries the summary packs to the same bytes as one without it, and the record length is the old one
    for a, b in zip(plain, with_smp):
        fa, ia = restarts._pack(a, N, M, len(brk_ids), 4, brk_ids, names)
        fb, ib = restarts._pack(b, N, M, len(brk_ids), 4, brk_ids, names, cn_samples=False)
        assert fa.tobytes() == fb.tobytes() and ia.tobytes() == ib.tobytes()
        assert len(fa) == restarts._HDR + M + 4 + 4 * N
    off = restarts.gather_result_records(plain, e, ps, M, names)
    for i, res in off.items():
        assert 'cn_sample_agreement' not in res and 'ploidy_q50' not in res['stats']
    on = restarts.gather_result_records(with_smp, e, ps, M, names, cn_samples=True)
    for i, res in on.items():
        src = with_smp[i]
        assert np.array_equal(res['cn_sample_agreement'], src['cn_sample_agreement'])
        assert np.array_equal(res['cn_state_agreement'], src['cn_state_agreement'])
        for k in sampling.SUMMARY_STATS:
            assert res['stats'][k] == src['stats'][k]
        assert np.array_equal(res['cn'], src['cn']) and res['stats']['elbo'] == src['stats']['elbo']
        assert np.array_equal(res['p_outlier_total'], off[i]['p_outlier_total'])


def test_add_sample_summary_uses_the_decoded_path():
    rng = np.random.RandomState(1)
    N, M = 11, 3
    cn = rng.randint(0, 4, size=(N, M, 2))
    samples = np.repeat(cn[None], 4, axis=0)
    samples[1, 3, 2, 0] += 1
    res = sampling.add_sample_summary({'cn': cn, 'stats': {}}, samples, rng.uniform(1, 2, size=N))
    assert res['cn_sample_agreement'].shape == (N, M) and res['cn_state_agreement'].shape == (N,)
    assert res['cn_sample_agreement'][3, 2] == 0.75 and res['cn_state_agreement'][3] == 0.75
    assert (np.delete(res['cn_state_agreement'], 3) == 1.).all()
    assert set(sampling.SUMMARY_STATS) <= set(res['stats'])
