"""Host side of the call confidence (remixt_amd/posteriors.py) and its numpy twin, without a GPU: the twin
against path enumeration, batch_call_confidence / batch_cn_logprob against a batch answered by the twin, the config
check, the distributed record with and without config cn_call_confidence, the oracle kernel module, the declarations."""
import itertools
import os
import re

import numpy as np
import pytest

from remixt_amd import defaults, posteriors, restarts, synthetic
from tests import call_twin, region_twin
from tests import helpers as H
from tests.test_cn_samples_records_cpu import _fake_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _enumerate(f, T, a, b, lab, ref, constrain):
    """log P(label(c_n) == label(ref_n) at every bound n of [a, b]) over every path of one chain, written from the event."""
    N, S = f.shape
    num = den = 0.
    for path in itertools.product(range(S), repeat=N):
        w = np.exp(sum(f[n, path[n]] for n in range(N)) + sum(T[n, path[n], path[n + 1]] for n in range(N - 1)))
        den += w
        if all(lab[n][path[n]] == lab[n][ref[n]] for n in range(a, b + 1) if constrain is None or constrain[n]):
            num += w
    with np.errstate(divide='ignore'):
        return float(np.log(num / den))


def test_twin_against_enumeration():
    rng = np.random.RandomState(5)
    N, S = 5, 3
    f = rng.normal(scale=2., size=(N, S))
    T = rng.normal(scale=2., size=(N - 1, S, S))
    twin = region_twin.RegionTwin(f, T, [0], [N - 1])
    identity = np.tile(np.arange(S), (N, 1))
    # the labels: the state itself (None: label -1), one table that merges two states, one per-segment table, one constant
    labels = [None, np.tile([0, 1, 0], (N, 1)), rng.randint(0, 2, size=(N, S)), np.zeros((N, S), dtype=int)]
    holes = np.array([1, 0, 1, 1, 0], dtype=bool)
    refs = [rng.randint(0, S, size=N) for _ in range(3)]
    runs = list(itertools.combinations_with_replacement(range(N), 2))
    worst = 0.
    for a, b in runs:
        for lab in labels:
            for constrain in (None, holes):
                for ref in refs:
                    got = call_twin.logprob(twin, a, b, lab, ref, constrain)
                    mask = call_twin.call_mask(lab, ref, S)
                    want = region_twin.brute_force(f, T, a, b, mask, None, constrain)
                    direct = _enumerate(f, T, a, b, identity if lab is None else lab, ref, constrain)
                    worst = max(worst, abs(np.exp(got) - np.exp(want)), abs(np.exp(got) - np.exp(direct)))
                    assert abs(np.exp(got) - np.exp(want)) <= 1e-12 and abs(np.exp(got) - np.exp(direct)) <= 1e-12, (a, b, ref)
    # a constant label allows everything; an unbound segment alone is certain
    assert abs(call_twin.logprob(twin, 0, N - 1, labels[3], refs[0])) <= 1e-12
    assert abs(call_twin.logprob(twin, 1, 1, None, refs[0], holes)) <= 1e-12
    # the whole chain, label -1, everything bound: the probability of the path itself
    ref = refs[1]
    w = sum(f[n, ref[n]] for n in range(N)) + sum(T[n, ref[n], ref[n + 1]] for n in range(N - 1))
    assert abs(call_twin.logprob(twin, 0, N - 1, None, ref) - float(w - twin.logZ[0])) <= 1e-12
    print('twin against enumeration: worst |P - enumeration| %.3e' % worst)


def _twin_batch(nr=2, seed=3):
    """Seven experiment segments in two chains; the model inserts zero-length segments at 2 and 6 (nine model segments)."""
    rng = np.random.RandomState(seed)
    cn_classes = np.zeros((1, 6, 2, 2), dtype=int)
    cn_classes[0, :, 0] = (1, 1)
    cn_classes[0, :, 1] = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2)]
    N1, S = 9, 6
    tel = np.array([0, 0, 0, 0, 1, 0, 0, 0, 0])
    fs = [rng.normal(scale=1.5, size=(N1, S)) for _ in range(nr)]
    Ts = []
    for _ in range(nr):
        T = rng.normal(scale=1.5, size=(N1 - 1, S, S))
        T[4] = 0.
        Ts.append(T)
    cs, ce = posteriors.chains_from_telomeres(tel)
    assert list(cs) == [0, 5] and list(ce) == [4, 8]
    b = call_twin.TwinBatch(cn_classes, np.zeros(N1, dtype=int), fs, Ts, cs, ce)
    fwd = np.array([0, 1, 3, 4, 5, 7, 8])
    orig = np.ones(N1, dtype=bool); orig[[2, 6]] = False
    return b, fwd, orig, tel


def test_batch_call_confidence():
    b, fwd, orig, tel = _twin_batch()
    rng = np.random.RandomState(0)
    states = rng.randint(0, 6, size=(2, 9))
    # across the chain end, holding the inserted segment 2, a single segment, holding the inserted segment 6
    regions = [(0, 6), (1, 2), (3, 3), (4, 5)]
    pieces = [[(0, 4), (5, 8)], [(1, 3)], [(4, 4)], [(5, 7)]]
    out = posteriors.batch_call_confidence(b, 0, 2, states, regions, fwd, orig, tel)
    assert b.calls == [(2, 1, 3 * 5)]                                    # one device call: every piece and label
    _, label_tab = posteriors.event_tables(b.cn_classes)
    assert sorted(out) == sorted(posteriors.CALL_ARRAYS) and posteriors.CALL_ARRAYS == ('p_call', 'p_call_unphased', 'p_call_total')
    for name, lb in posteriors.CALL_LABELS:
        lab = label_tab[b.seg_class, posteriors.LABEL_NAMES.index(lb)]
        assert out[name].shape == (2, 4) and ((out[name] >= 0) & (out[name] <= 1)).all()
        for r in range(2):
            for j, runs in enumerate(pieces):
                want = np.exp(sum(call_twin.logprob(b.twins[r], a, e, lab, states[r], orig) for a, e in runs))
                assert abs(out[name][r, j] - want) <= 1e-12, (name, r, j)
    assert (out['p_call'] <= out['p_call_unphased'] + 1e-12).all() and (out['p_call_unphased'] <= out['p_call_total'] + 1e-12).all()
    assert (out['p_call'] < out['p_call_total'] - 1e-6).any()
    # what the call holds at the inserted segments is ignored
    other = states.copy(); other[:, [2, 6]] = (other[:, [2, 6]] + 1) % 6
    again = posteriors.batch_call_confidence(b, 0, 2, other, regions, fwd, orig, tel)
    for k in out:
        assert np.array_equal(out[k], again[k]), k
    # restart range, and no regions: no device call
    one = posteriors.batch_call_confidence(b, 1, 1, states[1:], regions, fwd, orig, tel)
    assert all(np.array_equal(one[k][0], out[k][1]) for k in out)
    ncalls = len(b.calls)
    empty = posteriors.batch_call_confidence(b, 0, 2, states, [], fwd, orig, tel)
    assert all(empty[k].shape == (2, 0) for k in posteriors.CALL_ARRAYS) and len(b.calls) == ncalls


def test_batch_cn_logprob_and_chunking(monkeypatch):
    b, fwd, orig, tel = _twin_batch()
    rng = np.random.RandomState(1)
    K = 5
    states = rng.randint(0, 6, size=(2, K, 9))
    got = posteriors.batch_cn_logprob(b, 0, 2, states, orig, tel)
    assert got.shape == (2, K) and b.calls == [(2, K, K * 2)]
    for r in range(2):
        for k in range(K):
            want = sum(call_twin.logprob(b.twins[r], a, e, None, states[r, k], orig) for a, e in ((0, 4), (5, 8)))
            assert abs(got[r, k] - want) <= 1e-12 * max(1., abs(want)), (r, k)
    # a path without inserted segments bound equals the marginal over them: with everything bound it is less likely
    assert (posteriors.batch_cn_logprob(b, 0, 2, states, np.ones(9, dtype=bool), tel) < got).all()
    # chunks over K: at most two paths per restart and call
    b.calls = []
    monkeypatch.setattr(posteriors, '_CALL_PATH_BYTES', 2 * 2 * 9 * 2)
    chunked = posteriors.batch_cn_logprob(b, 0, 2, states, orig, tel)
    assert b.calls == [(2, 2, 4), (2, 2, 4), (2, 1, 2)] and np.array_equal(chunked, got)
    assert posteriors._CALL_PATH_BYTES == 72
    with pytest.raises(ValueError, match='must have shape'):
        posteriors.batch_cn_logprob(b, 0, 2, states[0], orig, tel)


def test_config():
    assert defaults.cn_call_confidence is False and defaults.get_param({}, 'cn_call_confidence') is False
    assert posteriors.call_confidence_on({}) is False and posteriors.call_confidence_on({'cn_regions': [('a', 0, 1)]}) is False
    assert posteriors.call_confidence_on({'cn_regions': [('a', 0, 1)], 'cn_call_confidence': True}) is True
    with pytest.raises(ValueError, match='cn_call_confidence needs cn_regions'):
        posteriors.call_confidence_on({'cn_call_confidence': True})
    # the entry points refuse it before any fit
    from remixt_amd.analysis import pipeline
    e = synthetic.make_experiment(20, num_clones=3, max_copy_number=3, num_chains=2, seed=0)
    ps = synthetic.make_init_params(e, 2, 3)
    with pytest.raises(ValueError, match='cn_call_confidence needs cn_regions'):
        pipeline.fit_restarts(e, dict(enumerate(ps)), {'cn_call_confidence': True})
    with pytest.raises(ValueError, match='cn_call_confidence needs cn_regions'):
        pipeline.fit(e, ps[0], {'cn_call_confidence': True})
    with pytest.raises(ValueError, match='cn_call_confidence needs cn_regions'):
        restarts.fit_restarts_distributed(e, ps, 3, cn_call_confidence=True)


def test_record_round_trip_and_unchanged_when_off():
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=4, num_chains=3, seed=2)
    ps = synthetic.make_init_params(e, 3, 4)
    rng = np.random.RandomState(0)
    names = ['negbin_r_0', 'negbin_r_1', 'betabin_M_0', 'betabin_M_1']
    N, M, K = len(e.x), 3, 5
    brk_ids = list(e.breakpoints.keys())
    region_names = ['geneA', 'arm', 'one']
    R = len(region_names)
    plain = [_fake_result(e, rng) for _ in ps]
    full = []
    for res in plain:
        r2 = dict(res, stats=dict(res['stats']))
        posteriors.add_region_events(r2, region_names, dict((k, rng.uniform(size=R)) for k in posteriors.REGION_ARRAYS))
        posteriors.add_region_change_counts(r2, region_names, K, dict((k, rng.dirichlet(np.ones(K), size=R)) for k in posteriors.COUNT_ARRAYS))
        posteriors.add_call_confidence(r2, region_names, dict((k, rng.uniform(size=R)) for k in posteriors.CALL_ARRAYS), -rng.uniform(1, 50))
        assert sorted(r2['call_confidence']) == ['names', 'p_call', 'p_call_total', 'p_call_unphased'] and r2['stats']['cn_logprob'] < 0
        full.append(r2)
    for a, b in zip(plain, full):
        fa, ia = restarts._pack(a, N, M, len(brk_ids), 4, brk_ids, names)
        # off (the default): the records of a run that never heard of it, with and without regions and counts
        fb, ib = restarts._pack(b, N, M, len(brk_ids), 4, brk_ids, names)
        assert fa.tobytes() == fb.tobytes() and ia.tobytes() == ib.tobytes()
        fn, _ = restarts._pack(b, N, M, len(brk_ids), 4, brk_ids, names, region_names=None, call_confidence=True)
        assert fn.tobytes() == fa.tobytes()
        for bins in (0, K):
            fr, ir = restarts._pack(b, N, M, len(brk_ids), 4, brk_ids, names, region_names=region_names, change_bins=bins)
            fr0, _ = restarts._pack(b, N, M, len(brk_ids), 4, brk_ids, names, region_names=region_names, change_bins=bins, call_confidence=False)
            assert fr.tobytes() == fr0.tobytes() and len(fr) == len(fa) + 7 * R + 2 * bins * R
            # on: 3 R + 1 slots, after everything else
            fc, ic = restarts._pack(b, N, M, len(brk_ids), 4, brk_ids, names, region_names=region_names, change_bins=bins, call_confidence=True)
            assert len(fc) == len(fr) + 3 * R + 1 and fc[:len(fr)].tobytes() == fr.tobytes() and ic.tobytes() == ir.tobytes()
            assert fc[-1] == b['stats']['cn_logprob'] and np.array_equal(fc[-1 - R:-1], b['call_confidence']['p_call_total'])
    off = restarts.gather_result_records(full, e, ps, M, names, region_names=region_names, change_bins=K)
    on = restarts.gather_result_records(full, e, ps, M, names, region_names=region_names, change_bins=K, call_confidence=True)
    for i, res in on.items():
        assert 'call_confidence' not in off[i] and 'cn_logprob' not in off[i]['stats']
        assert sorted(set(res) - {'call_confidence'}) == sorted(off[i]) and sorted(set(res['stats']) - {'cn_logprob'}) == sorted(off[i]['stats'])
        got = res['call_confidence']
        assert got['names'] == region_names and res['stats']['cn_logprob'] == full[i]['stats']['cn_logprob']
        for k in posteriors.CALL_ARRAYS:
            assert got[k].shape == (R,) and np.array_equal(got[k], full[i]['call_confidence'][k]), k
        for k in posteriors.REGION_ARRAYS:
            assert np.array_equal(res['region_events'][k], full[i]['region_events'][k]) and np.array_equal(off[i]['region_events'][k], res['region_events'][k]), k
        for k in posteriors.COUNT_ARRAYS:
            assert np.array_equal(res['region_change_counts'][k], full[i]['region_change_counts'][k]), k
        assert np.array_equal(res['cn'], full[i]['cn']) and res['stats']['elbo'] == full[i]['stats']['elbo']
    # next to the posterior summary block
    more = []
    for res in full:
        r3 = dict(res, stats=dict(res['stats']))
        summary = dict((k, rng.uniform(size=(N, M) if k.startswith('total_cn') else (N,))) for k in posteriors.COMPACT_ARRAYS)
        summary['expected_alleles_subclonal'] = rng.uniform(0, 2, size=N)
        posteriors.add_posterior_summary(r3, summary, e.l)
        more.append(r3)
    both = restarts.gather_result_records(more, e, ps, M, names, cn_posterior=True, region_names=region_names, call_confidence=True)
    for i, res in both.items():
        for k in posteriors.COMPACT_ARRAYS:
            assert np.array_equal(res[k], more[i][k]), k
        for k in posteriors.CALL_ARRAYS:
            assert np.array_equal(res['call_confidence'][k], more[i]['call_confidence'][k]), k
        assert res['stats']['cn_logprob'] == more[i]['stats']['cn_logprob']


def test_store_unchanged_when_off_and_arrays_when_on(tmp_path):
    from remixt_amd.analysis import pipeline
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=4, num_chains=3, seed=2)
    rng = np.random.RandomState(0)
    res = _fake_result(e, rng)
    res['h'] = np.array([0.1, 0.2, 0.3]); res['cn'] = np.ones((len(e.x), 3, 2), dtype=int)
    on = dict(res, stats=dict(res['stats']))
    posteriors.add_call_confidence(on, ['a', 'b'], dict((k, rng.uniform(size=2)) for k in posteriors.CALL_ARRAYS), -3.)
    keys = {}
    for tag, r in (('off', res), ('on', on)):
        with pipeline._Store(str(tmp_path / (tag + '.store')), 'w') as store:
            pipeline.store_fit_results(store, e, r, '/solutions/solution_0')
            keys[tag] = set(k.lstrip('/') for k in store.keys())
    extra = set('solutions/solution_0/' + k for k in posteriors.CALL_ARRAYS)
    assert keys['on'] - keys['off'] == extra and not (keys['off'] & extra)


def test_oracle_kernel_module():
    from oracle import oracle
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError, match='has no call probabilities'):
        mo.call_confidence([(0, 3)])
    with pytest.raises(NotImplementedError, match='has no call probabilities'):
        mo.cn_logprob()


def test_declarations():
    from remixt_amd import _lib
    assert 'rmx_call_prob' in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, 'include', 'remixt_amd.h')).read()
    m = re.search(r'int rmx_call_prob\(([^;]*)\);', hdr)
    assert m is not None
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    assert len(params) == 11 == len(_lib.SYMBOLS['rmx_call_prob'][1])
    assert params[3] == 'int32_t npaths' and params[4] == 'const int16_t *paths' and params[-1] == 'double *logp_out'
    src = open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_api.hip')).read()
    assert '"k_region_counts", "k_call_prob"' in src      # the profile table, beside k_region_counts
