"""Host side of the region decode (rmx_region_decode; remixt_amd/posteriors.py batch_region_calls) and its numpy twin,
without a GPU: the twin against path enumeration, the declarations, the records and result keys with the option off and
on, NotImplementedError over the oracle, and batch_region_calls against a batch answered by the twin.
test_twin_against_enumeration, test_twin_impossible_event and test_twin_chain_end run test-side code only: they check the reference the
device tests are held to, and pass with or without the feature; every other test here needs it."""
import os
import re

import numpy as np
import pytest

from remixt_amd import posteriors
from tests import call_twin, decode_twin, region_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chain(seed, N, S):
    rng = np.random.RandomState(seed)
    f = rng.normal(scale=2., size=(N, S))
    T = rng.normal(scale=2., size=(N - 1, S, S))
    masks = rng.uniform(size=(2, N, S)) < 0.6
    masks[:, :, 0] = True                               # (no segment without an allowed state)
    labels = np.stack([np.tile(np.arange(S), (N, 1)), np.array([[0, 1, 0, 1], [0, 0, 1, 1]])[np.arange(N) % 2][:, :S]])
    constrain = np.ones(N, dtype=bool); constrain[2] = False
    return f, T, masks, labels, constrain


# (N, S, a, b, mask index or -1, label index or -1): whole chains, runs inside one (messages on both sides), runs that
# touch a chain end, one segment, S = 2 .. 4
_CASES = [
    (6, 3, 0, 5, -1, -1), (6, 3, 1, 4, 0, -1), (6, 3, 1, 4, -1, 1), (6, 3, 0, 5, 1, 1), (6, 3, 2, 2, 0, -1), (6, 3, 2, 3, 1, 0),
    (5, 4, 0, 2, 0, 1), (5, 4, 2, 4, -1, 1), (5, 4, 1, 3, 1, -1), (6, 2, 0, 5, 0, 1), (6, 2, 3, 5, -1, 0), (4, 4, 0, 3, -1, -1),
]


@pytest.mark.parametrize('case', range(len(_CASES)))
@pytest.mark.parametrize('use_constrain', [False, True])
def test_twin_against_enumeration(case, use_constrain):
    N, S, a, b, mi, li = _CASES[case]
    f, T, masks, labels, constrain = _chain(20 + case, N, S)
    cs = constrain if use_constrain else None
    mk, lb = (None if mi < 0 else masks[mi]), (None if li < 0 else labels[li])
    twin = region_twin.RegionTwin(f, T, [0], [N - 1])
    got, path = decode_twin.decode(twin, a, b, mk, lb, cs)
    want, best = decode_twin.brute_force(f, T, a, b, mk, lb, cs)
    print('case %d: twin %.17g enumerated %.17g, path %s' % (case, got, want, path))
    assert np.isfinite(want) and abs(got - want) <= 1e-12
    assert tuple(int(s) for s in path) in best and decode_twin.satisfies(path, a, b, mk, lb, cs)
    # the path's own log-probability, by the call twin, is the optimum; and the maximum is not above the sum
    assert abs(call_twin.logprob(twin, a, b, None, np.concatenate([np.zeros(a, dtype=int), path, np.zeros(N - 1 - b, dtype=int)])) - got) <= 1e-12
    assert got <= twin.logprob(a, b, mk, lb, cs) + 1e-12


def test_twin_impossible_event():
    f, T, masks, labels, _ = _chain(3, 5, 3)
    masks = masks.copy()
    masks[0, 3] = False                                  # no state of segment 3 is allowed
    twin = region_twin.RegionTwin(f, T, [0], [4])
    assert decode_twin.brute_force(f, T, 2, 4, masks[0], None) == (-np.inf, set())
    assert decode_twin.decode(twin, 2, 4, masks[0], None) == (-np.inf, None)
    cs = np.ones(5, dtype=bool); cs[3] = False          # ... and not where the segment does not bind
    assert np.isfinite(decode_twin.decode(twin, 2, 4, masks[0], None, cs)[0])


def test_twin_chain_end():
    """Two chains in one model: a run of the second chain starts from its own first segment, not from the first chain."""
    rng = np.random.RandomState(5)
    N, S = 6, 3
    f, T = rng.normal(scale=2., size=(N, S)), rng.normal(scale=2., size=(N - 1, S, S))
    T[2] = 0.
    twin = region_twin.RegionTwin(f, T, [0, 3], [2, 5])
    got, path = decode_twin.decode(twin, 3, 5)
    want, best = decode_twin.brute_force(f[3:], T[3:], 0, 2)
    assert abs(got - want) <= 1e-12 and tuple(int(s) for s in path) in best
    got, path = decode_twin.decode(twin, 1, 2)
    want, best = decode_twin.brute_force(f[:3], T[:2], 1, 2)
    assert abs(got - want) <= 1e-12 and tuple(int(s) for s in path) in best


# the kernel names of the parent commit, in id order
_PARENT_KERNELS = [
    'k_state_tables', 'k_seg_const', 'k_framelogprob', 'k_fb', 'k_marginals<true>', 'k_marginals<false>', 'k_update_outlier_total',
    'k_update_outlier_allele', 'k_update_allele_swap', 'k_brk_lut', 'k_pairwise', 'k_brk_update', 'k_elbo_seg', 'k_elbo_final',
    'k_ell_list', 'k_ell_final', 'k_ell_full', 'k_viterbi', 'k_backtrace', 'other', 'k_sample_cn', 'k_posterior_summary', 'k_region_prob',
    'k_region_counts', 'k_call_prob', 'k_region_moments', 'k_region_extent', 'k_region_span', 'k_region_pattern']


def test_declared_and_bound():
    from remixt_amd import _lib, bpmodel, cn_model, restarts
    assert 'rmx_region_decode' in _lib.SYMBOLS and len(_lib.SYMBOLS['rmx_region_decode'][1]) == 13
    with open(os.path.join(ROOT, 'include', 'remixt_amd.h')) as fh:
        text = re.sub(r'\s+', ' ', fh.read())
    assert ('int rmx_region_decode(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t nmask, '
            'const uint8_t *masks, int32_t nlabel, const int16_t *labels, const uint8_t *constrain, int32_t max_len, '
            'int16_t *states_out, double *logp_out);') in text
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_api.hip')) as fh:
        api = fh.read()
    # profile ids are appended: the parent's names are a prefix of the list, the new one comes right after k_region_pattern
    names = re.findall(r'"([^"]*)"', re.search(r'kKernelNames\[KID_COUNT\] = \{(.*?)\};', api, re.S).group(1))
    assert names[:len(_PARENT_KERNELS)] == _PARENT_KERNELS and names[len(_PARENT_KERNELS)] == 'k_region_decode'
    ids = [t.strip().split(' ')[0] for t in re.search(r'enum KernelId \{(.*?)\};', api, re.S).group(1).split(',')]
    assert ids[-1] == 'KID_COUNT' and len(ids) == len(names) + 1
    assert ids[names.index('k_region_decode')] == 'KID_REGION_DECODE' and ids[names.index('k_region_pattern')] == 'KID_REGION_PATTERN'
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_host.h')) as fh:
        host = fh.read()
    assert 'inline int64_t check_decode_lengths(' in host and 'inline int decode_plan(' in host
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_kernels.h')) as fh:
        kern = fh.read()
    assert kern.index('void k_region_decode(') > kern.index('void k_region_pattern(')
    assert hasattr(bpmodel.RemixtBatch, 'region_decode_raw') and hasattr(bpmodel.RemixtModel, 'region_decode')
    for cls in (cn_model.BreakpointModel, restarts.RestartSet, restarts.RestartGroups, restarts.DatasetGroups):
        assert hasattr(cls, 'region_call'), cls


def test_records_and_config_unchanged_when_off():
    from remixt_amd import defaults, restarts, synthetic
    from tests.test_cn_samples_records_cpu import _fake_result
    assert defaults.cn_region_calls is False and defaults.get_param({}, 'cn_region_calls') is False
    assert posteriors.region_calls_on({}) is False and posteriors.region_calls_on({'cn_region_calls': True, 'cn_regions': [('a', 0, 1)]}) is True
    with pytest.raises(ValueError):
        posteriors.region_calls_on({'cn_region_calls': True})
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=4, num_chains=3, seed=2)
    ps = synthetic.make_init_params(e, 3, 4)
    rng = np.random.RandomState(0)
    names = ['negbin_r_0', 'negbin_r_1', 'betabin_M_0', 'betabin_M_1']
    N, M = len(e.x), 3
    brk_ids = list(e.breakpoints.keys())
    K = len(brk_ids)
    regions = ['arm', 'gene', 'focal', 'tail']
    R = len(regions)
    full = []
    for _ in ps:
        res = _fake_result(e, rng)
        keys = sorted(res)
        posteriors.add_region_events(res, regions, dict((k, rng.uniform(size=R)) for k in posteriors.REGION_ARRAYS))
        with_events = sorted(res)
        posteriors.add_region_calls(res, regions, {'log_prob': -rng.uniform(size=R), 'log_prob_call': -rng.uniform(size=R), 'n_differ': rng.randint(0, 5, size=R)})
        assert sorted(set(res) - {'region_calls'}) == with_events and sorted(set(res) - {'region_calls', 'region_events'}) == keys
        assert len(posteriors.REGION_CALL_ARRAYS) == 3 and res['region_calls']['names'] == regions
        full.append(res)
    for res in full:
        f0, i0 = restarts._pack(res, N, M, K, 4, brk_ids, names, region_names=regions)
        f1, i1 = restarts._pack(res, N, M, K, 4, brk_ids, names, region_names=regions, region_calls=False)
        assert f0.tobytes() == f1.tobytes() and i0.tobytes() == i1.tobytes()
        f2, i2 = restarts._pack(res, N, M, K, 4, brk_ids, names, region_names=regions, region_calls=True)
        assert len(f2) == len(f0) + 3 * R and f2[:len(f0)].tobytes() == f0.tobytes() and i2.tobytes() == i0.tobytes()
        assert np.array_equal(f2[len(f0):], np.concatenate([res['region_calls'][k] for k in posteriors.REGION_CALL_ARRAYS]))
        # without regions there is nothing to add, and the record without either is the record of a build without the option
        f3, _ = restarts._pack(res, N, M, K, 4, brk_ids, names)
        f4, _ = restarts._pack(res, N, M, K, 4, brk_ids, names, region_calls=True)
        assert f3.tobytes() == f4.tobytes() and len(f3) == len(f0) - len(posteriors.REGION_ARRAYS) * R
    off = restarts.gather_result_records(full, e, ps, M, names, region_names=regions)
    on = restarts.gather_result_records(full, e, ps, M, names, region_names=regions, region_calls=True)
    for i, res in on.items():
        assert sorted(set(res) - {'region_calls'}) == sorted(off[i]) and 'region_calls' not in off[i]
        assert res['region_calls']['names'] == regions
        for k in posteriors.REGION_CALL_ARRAYS:
            assert res['region_calls'][k].shape == (R,) and np.array_equal(res['region_calls'][k], full[i]['region_calls'][k]), k
        for k in off[i]:
            if isinstance(off[i][k], np.ndarray):
                assert np.array_equal(off[i][k], res[k], equal_nan=True), k


def test_no_region_call_without_the_kernel():
    from oracle import oracle
    from tests import helpers as H
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError):
        mo.region_call([(1, 2)])
    with pytest.raises(NotImplementedError):
        mo.region_call([(1, 2)], ('loh', None))


def _twin_batch(nr=2, seed=4):
    """Twelve model segments in two chains (chain ends after 5 and 11), six states of three clones: states 0, 1 and 4 are
    LOH, 0 is a homozygous deletion, 2 and 5 are subclonal, 3 .. 5 share their totals."""
    rng = np.random.RandomState(seed)
    S, M = 6, 3
    cn_classes = np.zeros((1, S, M, 2), dtype=int)
    cn_classes[0, :, 1] = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (1, 1)]
    cn_classes[0, :, 2] = [(0, 0), (1, 0), (1, 1), (1, 1), (2, 0), (0, 2)]
    N1 = 12
    tel = np.zeros(N1, dtype=int); tel[[5, 11]] = 1
    fs = [rng.normal(scale=1.5, size=(N1, S)) for _ in range(nr)]
    Ts = []
    for _ in range(nr):
        T = rng.normal(scale=1.5, size=(N1 - 1, S, S))
        T[5] = 0.
        Ts.append(T)
    cs, ce = posteriors.chains_from_telomeres(tel)
    return decode_twin.DecodeTwinBatch(cn_classes, np.zeros(N1, dtype=int), fs, Ts, cs, ce), tel


def test_region_calls_over_the_twin():
    b, tel = _twin_batch()
    # ten experiment segments; model segments 3 and 8 are inserted ones
    fwd, orig = np.array([0, 1, 2, 4, 5, 6, 7, 9, 10, 11]), np.ones(12, dtype=bool)
    orig[[3, 8]] = False
    masks, labels = posteriors.event_tables(b.cn_classes)
    mk = masks[0][:, None, :].repeat(12, axis=1) != 0
    lb = labels[0][:, None, :].repeat(12, axis=1)
    nloh, tot = posteriors.MASK_NAMES.index('not_loh'), posteriors.LABEL_NAMES.index('total')
    # regions: inside chain 0 across the inserted segment; across the chain end (experiment 4 | 5); one segment; named
    regions = [(1, 3), (3, 6), (7, 7), ('tail', 8, 9)]
    runs = [[(1, 4)], [(4, 5), (6, 7)], [(9, 9)], [(10, 11)]]
    rng = np.random.RandomState(1)
    call = rng.randint(0, 6, size=(2, 12))
    out = posteriors.batch_region_calls(b, 0, 2, regions, fwd, orig, tel)
    assert [c[0] for c in b.calls] == ['region_decode'] and b.calls[0][1:] == (2, 5)
    assert sorted(out) == ['cn', 'log_p_event', 'log_prob', 'log_prob_given_event']
    assert (out['log_p_event'] == 0).all() and np.array_equal(out['log_prob_given_event'], out['log_prob'])
    for event, mi, li in ((None, -1, -1), (('not_loh', None), nloh, -1), ((None, 'total'), -1, tot), (('not_loh', 'total'), nloh, tot)):
        del b.calls[:]
        out = posteriors.batch_region_calls(b, 0, 2, regions, fwd, orig, tel, event=event, cn=call)
        assert [c[0] for c in b.calls] == ['region_decode'] + (['region_logprob'] if event else []) + ['call_logprob']
        assert out['log_prob'].shape == (2, 4) and out['n_differ'].shape == (2, 4) and len(out['cn']) == 2 and len(out['cn'][0]) == 4
        for r in range(2):
            tw = b.twins[r]
            for k, pieces in enumerate(runs):
                dec = [decode_twin.decode(tw, a, z, None if mi < 0 else mk[mi], None if li < 0 else lb[li], orig) for a, z in pieces]
                assert abs(out['log_prob'][r, k] - sum(d[0] for d in dec)) <= 1e-12
                ev = sum(tw.logprob(a, z, None if mi < 0 else mk[mi], None if li < 0 else lb[li], orig) for a, z in pieces) if event else 0.
                assert abs(out['log_p_event'][r, k] - min(ev, 0.)) <= 1e-12
                assert out['log_prob_given_event'][r, k] <= 0 and abs(out['log_prob_given_event'][r, k] - (out['log_prob'][r, k] - out['log_p_event'][r, k])) <= 1e-12
                # the copy numbers of the region's own segments: the inserted model segment 3 of region 0 is not among them
                first, last = regions[k][-2:]
                seg = fwd[first:last + 1]
                full = np.full(12, -1)
                for (a, z), d in zip(pieces, dec):
                    full[a:z + 1] = d[1]
                assert out['cn'][r][k].shape == (len(seg), 3, 2) and np.array_equal(out['cn'][r][k], b.cn_classes[0, full[seg]])
                assert out['n_differ'][r, k] == (full[seg] != call[r, seg]).sum()
                # a mask binds the original segments only
                if mi >= 0:
                    assert all(mk[mi][n, full[n]] for n in seg)
                want = sum(call_twin.logprob(tw, a, z, lb[posteriors.LABEL_NAMES.index('state')], call[r], orig) for a, z in pieces)
                assert abs(out['log_prob_call'][r, k] - min(want, 0.)) <= 1e-12
    # the twin's own configuration as the call: it differs nowhere, and where the region holds no inserted segment the call's
    # log-probability is the configuration's
    dec = posteriors.batch_region_calls(b, 0, 2, regions, fwd, orig, tel)
    for k, pieces in enumerate(runs):
        st = np.zeros((2, 12), dtype=int)
        for r in range(2):
            for a, z in pieces:
                st[r, a:z + 1] = decode_twin.decode(b.twins[r], a, z, None, None, orig)[1]
        same = posteriors.batch_region_calls(b, 0, 2, regions[k:k + 1], fwd, orig, tel, cn=st)
        assert (same['n_differ'] == 0).all() and np.array_equal(same['log_prob'][:, 0], dec['log_prob'][:, k])
        if k == 0:      # (the inserted segment 3 is summed out in the call's probability)
            assert (same['log_prob_call'][:, 0] >= dec['log_prob'][:, 0] - 1e-12).all()
        else:
            assert np.abs(same['log_prob_call'][:, 0] - dec['log_prob'][:, k]).max() <= 1e-12
    # no regions
    none = posteriors.batch_region_calls(b, 0, 2, [], fwd, orig, tel, cn=call)
    assert none['log_prob'].shape == (2, 0) and none['n_differ'].shape == (2, 0) and none['cn'] == [[], []]
    with pytest.raises(ValueError):
        posteriors.batch_region_calls(b, 0, 2, regions, fwd, orig, tel, event=('nonsense', None))
