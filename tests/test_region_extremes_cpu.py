"""Host side of the region extremes (remixt_amd/posteriors.py) and their numpy twin, without a GPU: the twin against
brute-force path enumeration, the level tables against a direct loop over cn_classes, the per-column combination of a
region split at a chain end, pmf and quantile extraction, amplification_prob, the symbol, header and kernel id lists,
the distributed record with and without config cn_region_extremes, and the config checks."""
import itertools
import os
import re

import numpy as np
import pytest

from remixt_amd import defaults, posteriors, restarts, synthetic
from tests import extremes_twin, region_twin
from tests.test_cn_samples_records_cpu import _fake_result

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_twin_against_enumeration():
    """S <= 4, N <= 6: with and without a mask, constrain with holes, runs from the chain start and to the chain end."""
    rng = np.random.RandomState(17)
    N, S = 6, 3
    f = rng.normal(scale=2., size=(N, S))
    T = rng.normal(scale=2., size=(N - 1, S, S))
    twin = region_twin.RegionTwin(f, T, [0], [N - 1])
    mask = rng.uniform(size=(N, S)) < 0.6
    mask[np.arange(N), rng.randint(0, S, size=N)] = True
    level = rng.randint(0, 4, size=(N, S))
    level[2] = [3, 3, 0]                     # one state in the low columns
    level[4] = [2, 2, 2]                     # nothing below column 2: -inf there for every run through segment 4
    holes = np.array([1, 0, 1, 1, 0, 1], dtype=bool)
    cases = [dict(), dict(mask=mask), dict(constrain=holes), dict(mask=mask, constrain=holes)]
    runs = list(itertools.combinations_with_replacement(range(N), 2))
    assert (0, 3) in runs and (2, N - 1) in runs and (0, N - 1) in runs
    impossible = unbound = 0
    for a, b in runs:
        for kw in cases:
            for K in (1, 3, 5):
                want = extremes_twin.brute_force(f, T, a, b, K, level, **kw)
                got = extremes_twin.logcolumns(twin, a, b, K, level, **kw)
                assert got.shape == (K,)
                assert np.array_equal(got == -np.inf, want == -np.inf), (a, b, K, sorted(kw), got, want)
                assert (np.abs(np.exp(got) - np.exp(want)) <= 1e-12).all(), (a, b, K, sorted(kw), got, want)
                assert (np.diff(got[got > -np.inf]) >= -1e-12).all()                  # nested events
                impossible += int((want == -np.inf).sum())
            # a level >= ncol is in no column, and the last column of a table clipped to the window is the mask-only event
            clipped = extremes_twin.logcolumns(twin, a, b, 3, np.minimum(level, 2), **kw)
            assert abs(clipped[2] - twin.logprob(a, b, kw.get('mask'), None, kw.get('constrain'))) <= 1e-12
            if a <= 4 <= b:
                # segment 4 admits nothing below column 2 where it binds; alone and unbound it constrains nothing
                col = extremes_twin.logcolumns(twin, a, b, 2, level, **kw)
                if kw.get('constrain') is None:
                    assert (col == -np.inf).all()
                elif a == b:
                    assert (np.abs(col) <= 1e-12).all()
                    unbound += 1
    assert impossible >= 20 and unbound == 2
    # four states, a short chain
    f4, T4 = rng.normal(size=(4, 4)), rng.normal(size=(3, 4, 4))
    lv4 = rng.randint(0, 3, size=(4, 4))
    t4 = region_twin.RegionTwin(f4, T4, [0], [3])
    for a, b in ((0, 3), (1, 2), (3, 3)):
        assert np.abs(np.exp(extremes_twin.logcolumns(t4, a, b, 3, lv4)) - np.exp(extremes_twin.brute_force(f4, T4, a, b, 3, lv4))).max() <= 1e-12


def test_twin_with_two_chains():
    rng = np.random.RandomState(6)
    S = 3
    f = rng.normal(size=(7, S)); T = rng.normal(size=(6, S, S))
    T[3] = 0.      # (the adjacency across the chain end, as log_transmat holds it)
    both = region_twin.RegionTwin(f, T, [0, 4], [3, 6])
    level = rng.randint(0, 3, size=(7, S))
    assert np.abs(np.exp(extremes_twin.logcolumns(both, 1, 3, 3, level)) - np.exp(extremes_twin.brute_force(f[:4], T[:3], 1, 3, 3, level[:4]))).max() <= 1e-12
    assert np.abs(np.exp(extremes_twin.logcolumns(both, 4, 6, 3, level)) - np.exp(extremes_twin.brute_force(f[4:], T[4:], 0, 2, 3, level[4:]))).max() <= 1e-12


def _classes(rng, C=2, S=9, M=4, top=7):
    cn = rng.randint(0, top, size=(C, S, M, 2))
    cn[:, :, 0, :] = 1
    return cn


def test_level_tables():
    rng = np.random.RandomState(2)
    cn = _classes(rng)
    C, S, M, _ = cn.shape
    for ncol, first in ((16, 0), (5, 0), (4, 3), (1, 0)):
        levels, names = posteriors.level_tables(cn, ncol, first)
        assert levels.dtype == np.int16 and levels.shape == (C, 2 * 3 * M, S) and len(names) == len(set(names)) == 2 * 3 * M
        assert levels.flags['C_CONTIGUOUS'] and levels.min() >= 0 and levels.max() <= ncol - 1
        assert names[:M] == ['peak_total_1', 'peak_total_2', 'peak_total_3', 'peak_total_any'] and names[-1] == 'floor_minor_any'
        for c in range(C):
            for s in range(S):
                for quantity, fn in (('total', sum), ('major', max), ('minor', min)):
                    per = [fn(int(x) for x in cn[c, s, m]) for m in range(1, M)]
                    for clone, hi, lo in [(m, per[m - 1], per[m - 1]) for m in range(1, M)] + [('any', max(per), min(per))]:
                        wp = min(max(hi - first, 0), ncol - 1)
                        wf = min(max(lo - first, 0), ncol - 1)
                        assert levels[c, names.index(posteriors.level_name('peak', quantity, clone)), s] == wp
                        assert levels[c, names.index(posteriors.level_name('floor', quantity, clone)), s] == ncol - 1 - wf      # the reflection
    # two state classes that differ in a tumour row get different tables; the normal row does not matter
    levels, names = posteriors.level_tables(cn, 16)
    other = cn.copy(); other[:, :, 0, :] = (1, 0)
    assert not np.array_equal(levels[0], levels[1]) and np.array_equal(posteriors.level_tables(other, 16)[0], levels)
    # "every level' <= j" under the reflected table is "every q >= first + ncol - 1 - j"
    ncol, first = 6, 1
    levels, names = posteriors.level_tables(cn, ncol, first)
    q = cn[:, :, 2, :].sum(axis=-1)
    fl = levels[:, names.index('floor_total_2')]
    for j in range(ncol):
        k = ncol - 1 - j
        assert np.array_equal(fl <= j, (q >= first + k) if k > 0 else np.ones_like(q, dtype=bool))
    for bad in (dict(ncol=0), dict(ncol=17), dict(ncol=4, first_level=-1)):
        with pytest.raises(ValueError):
            posteriors.level_tables(cn, **bad)
    with pytest.raises(ValueError):
        posteriors.level_tables(cn[:, :, :1], 4)
    with pytest.raises(ValueError, match='quantity'):
        posteriors.level_name('peak', 'depth', 1)
    with pytest.raises(ValueError, match='orientation'):
        posteriors.level_name('top', 'total', 1)


def test_combine_columns_across_a_chain_end():
    """Two chains in one enumeration: a region over both is the product of its pieces, column by column."""
    rng = np.random.RandomState(4)
    S, K = 3, 4
    f = rng.normal(size=(5, S)); T = rng.normal(size=(4, S, S))
    T[2] = 0.                                                            # chains [0, 2] and [3, 4]: no coupling across
    level = rng.randint(0, 4, size=(5, S))
    level[3] = [3, 3, 1]                                                 # column 0 impossible in the second chain
    twin = region_twin.RegionTwin(f, T, [0, 3], [2, 4])
    pieces = np.stack([extremes_twin.logcolumns(twin, 1, 2, K, level), extremes_twin.logcolumns(twin, 3, 4, K, level),
                       extremes_twin.logcolumns(twin, 0, 0, K, level)])
    got = posteriors.combine_columns(pieces, [0, 0, 1], 3)
    assert got.shape == (3, K)
    # all five segments as one chain whose middle adjacency has weight 1 for every pair: the two chains side by side
    want = extremes_twin.brute_force(f, T, 1, 4, K, level)
    assert got[0, 0] == -np.inf and want[0] == -np.inf
    assert np.abs(np.exp(got[0]) - np.exp(want)).max() <= 1e-12
    assert np.array_equal(got[1], pieces[2]) and np.array_equal(got[2], np.zeros(K))      # one piece: itself; no piece: certain
    two = posteriors.combine_columns(np.stack([pieces, pieces[::-1]]), [0, 0, 1], 2)
    assert two.shape == (2, 2, K) and np.array_equal(two[0], got[:2]) and np.array_equal(two[1, 1], pieces[0])


def test_summary():
    # a CDF that dips by an ulp is clipped, not negative; a sum of logs an ulp above 0 is 1
    cdf = np.array([[0.25, 0.25 - 2. ** -54, 0.75, 1.0 + 2. ** -52], [0., 0., 0., 1.], [1., 1., 1., 1.]])
    surv = np.array([[1., 0.5, 0.5 + 2. ** -53, 0.], [1., 1., 1., 1.], [1., 0., 0., 0.]])
    with np.errstate(divide='ignore'):
        out = posteriors.extremes_summary(np.log(cdf), np.log(surv), first_level=2)
    assert out['bins'] == 4 and out['first_level'] == 2
    for k in ('peak_pmf', 'floor_pmf', 'peak_cdf', 'floor_cdf'):
        assert out[k].shape == (3, 4) and (out[k] >= 0).all() and (out[k] <= 1).all(), k
    assert out['peak_pmf'][0, 1] == 0 and out['floor_pmf'][0, 1] == 0 and out['peak_cdf'][0, 3] == 1
    assert np.abs(out['peak_pmf'][0] - [0.25, 0, 0.5, 0.25]).max() <= 1e-15 and np.abs(out['floor_pmf'][0] - [0.5, 0, 0.5, 0]).max() <= 1e-15
    # a saturated bin is reported as its edge: all of the peak in "5 or more" -> 5; all of the lowest value in "2 or less" -> 2
    assert np.array_equal(out['peak_pmf'][1], [0, 0, 0, 1]) and [out['peak_q%s' % q][1] for q in ('05', '50', '95')] == [5, 5, 5]
    assert np.array_equal(out['floor_pmf'][2], [1, 0, 0, 0]) and [out['floor_q%s' % q][2] for q in ('05', '50', '95')] == [2, 2, 2]
    assert np.array_equal(out['floor_pmf'][1], [0, 0, 0, 1]) and out['floor_q05'][1] == 5
    assert [out['peak_q%s' % q][0] for q in ('05', '50', '95')] == [2, 4, 5]
    assert [out['floor_q%s' % q][0] for q in ('05', '50', '95')] == [2, 2, 4]
    assert out['peak_q50'].dtype.kind == 'i'
    # an impossible mask-only event: nothing anywhere, no NaN
    with np.errstate(divide='ignore'):
        none = posteriors.extremes_summary(np.full((1, 3), -np.inf), np.full((1, 3), -np.inf))
    assert not np.isnan(none['peak_pmf']).any() and (none['peak_pmf'] == 0).all()


def test_amplification_prob():
    cdf = np.array([[0.1, 0.4, 0.9, 1.0]])
    with np.errstate(divide='ignore'):
        ex = posteriors.extremes_summary(np.log(cdf), np.log(cdf[:, ::-1]), first_level=3)
    assert np.allclose(posteriors.amplification_prob(ex, 4), [0.9], rtol=0, atol=1e-15)        # 1 - P(peak <= 3)
    assert np.allclose(posteriors.amplification_prob(ex, 6), [0.1], rtol=0, atol=1e-15)
    assert np.array_equal(posteriors.amplification_prob(ex, 0), [1.])
    for outside in (3, 7, 1):
        with pytest.raises(ValueError, match='first_level'):
            posteriors.amplification_prob(ex, outside)


# the kernel names of the parent commit, in id order
_PARENT_KERNELS = [
    'k_state_tables', 'k_seg_const', 'k_framelogprob', 'k_fb', 'k_marginals<true>', 'k_marginals<false>', 'k_update_outlier_total',
    'k_update_outlier_allele', 'k_update_allele_swap', 'k_brk_lut', 'k_pairwise', 'k_brk_update', 'k_elbo_seg', 'k_elbo_final',
    'k_ell_list', 'k_ell_final', 'k_ell_full', 'k_viterbi', 'k_backtrace', 'other', 'k_sample_cn', 'k_posterior_summary', 'k_region_prob',
    'k_region_counts', 'k_call_prob', 'k_region_moments', 'k_region_extent', 'k_region_span', 'k_region_pattern', 'k_region_decode']


def test_declared_and_bound():
    from remixt_amd import _lib, bpmodel, cn_model
    assert 'rmx_region_extremes' in _lib.SYMBOLS and len(_lib.SYMBOLS['rmx_region_extremes'][1]) == 12
    with open(os.path.join(ROOT, 'include', 'remixt_amd.h')) as fh:
        text = re.sub(r'\s+', ' ', fh.read())
    assert ('int rmx_region_extremes(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t nmask, '
            'const uint8_t *masks, int32_t nlevel, const int16_t *levels, const uint8_t *constrain, int32_t ncol, double *logp_out);') in text
    assert 'DESIGN 4.18' in text
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_api.hip')) as fh:
        api = fh.read()
    # profile ids are appended: the parent's names are a prefix of the list, the new one comes right after k_region_decode and is the last
    names = re.findall(r'"([^"]*)"', re.search(r'kKernelNames\[KID_COUNT\] = \{(.*?)\};', api, re.S).group(1))
    assert names[:len(_PARENT_KERNELS)] == _PARENT_KERNELS and names[len(_PARENT_KERNELS):] == ['k_region_extremes']
    ids = [t.strip().split(' ')[0] for t in re.search(r'enum KernelId \{(.*?)\};', api, re.S).group(1).split(',')]
    assert ids[-1] == 'KID_COUNT' and len(ids) == len(names) + 1
    assert ids[names.index('k_region_extremes')] == 'KID_REGION_EXTREMES' and ids[names.index('k_region_decode')] == 'KID_REGION_DECODE'
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_host.h')) as fh:
        host = fh.read()
    assert 'inline int64_t check_levels(' in host and 'inline bool extremes_ncol_ok(' in host
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_kernels.h')) as fh:
        kern = fh.read()
    assert kern.index('void k_region_extremes(') > kern.index('void k_region_counts(')
    body = kern[kern.index('void k_region_extremes('):kern.index('// Call probabilities:')]
    assert body.count('__builtin_amdgcn_mfma_f64_16x16x4f64(') == 1 and 'atomicAdd' not in body and 'asm' not in body
    assert hasattr(bpmodel.RemixtBatch, 'region_extremes_raw') and hasattr(bpmodel.RemixtModel, 'region_extremes')
    for cls in (cn_model.BreakpointModel, restarts.RestartSet, restarts.RestartGroups, restarts.DatasetGroups):
        assert hasattr(cls, 'region_cn_extremes') and hasattr(cls, 'region_clone_extremes'), cls


def test_records_and_config():
    assert defaults.cn_region_extremes is False and defaults.get_param({}, 'cn_region_extremes') is False
    assert posteriors.region_extremes_on({}) is False and posteriors.region_extremes_on({'cn_region_extremes': True, 'cn_regions': [('a', 0, 1)]}) is True
    with pytest.raises(ValueError, match='needs cn_regions'):
        posteriors.region_extremes_on({'cn_region_extremes': True})
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=4, num_chains=3, seed=2)
    ps = synthetic.make_init_params(e, 3, 4)
    rng = np.random.RandomState(0)
    names = ['negbin_r_0', 'negbin_r_1', 'betabin_M_0', 'betabin_M_1']
    N, M = len(e.x), 3
    brk_ids = list(e.breakpoints.keys())
    K = len(brk_ids)
    regions = ['arm', 'gene', 'focal', 'tail']
    R, B = len(regions), posteriors.EXTREME_BINS
    assert B == 16 and posteriors.EXTREME_ARRAYS == ('peak_total_pmf', 'floor_total_pmf')
    full = []
    for _ in ps:
        res = _fake_result(e, rng)
        keys = sorted(res)
        posteriors.add_region_events(res, regions, dict((k, rng.uniform(size=R)) for k in posteriors.REGION_ARRAYS))
        with_events = sorted(res)
        posteriors.add_region_cn_extremes(res, regions, dict((k, rng.dirichlet(np.ones(B), size=(R, M - 1))) for k in posteriors.EXTREME_ARRAYS))
        assert sorted(set(res) - {'region_cn_extremes'}) == with_events and sorted(set(res) - {'region_cn_extremes', 'region_events'}) == keys
        assert sorted(res['region_cn_extremes']) == ['bins', 'floor_total_pmf', 'names', 'peak_total_pmf']
        assert res['region_cn_extremes']['names'] == regions and res['region_cn_extremes']['bins'] == B
        full.append(res)
    for res in full:
        # off: the record of a build without the option, byte for byte
        f0, i0 = restarts._pack(res, N, M, K, 4, brk_ids, names, region_names=regions)
        f1, i1 = restarts._pack(res, N, M, K, 4, brk_ids, names, region_names=regions, region_extremes=False)
        assert f0.tobytes() == f1.tobytes() and i0.tobytes() == i1.tobytes()
        # on: 2 (M - 1) bins slots per region, at the end
        f2, i2 = restarts._pack(res, N, M, K, 4, brk_ids, names, region_names=regions, region_extremes=True)
        assert len(f2) == len(f0) + 2 * (M - 1) * B * R and f2[:len(f0)].tobytes() == f0.tobytes() and i2.tobytes() == i0.tobytes()
        assert np.array_equal(f2[len(f0):], np.concatenate([res['region_cn_extremes'][k].ravel() for k in posteriors.EXTREME_ARRAYS]))
        # pack / unpack round trip of the new section
        back = restarts._unpack(f2, i2, N, M, K, 4, brk_ids, names, ps[0], region_names=regions, region_extremes=True)
        for k in posteriors.EXTREME_ARRAYS:
            assert back['region_cn_extremes'][k].shape == (R, M - 1, B) and np.array_equal(back['region_cn_extremes'][k], res['region_cn_extremes'][k]), k
        assert back['region_cn_extremes']['names'] == regions and back['region_cn_extremes']['bins'] == B
        # without regions there is nothing to add
        f3, _ = restarts._pack(res, N, M, K, 4, brk_ids, names)
        f4, _ = restarts._pack(res, N, M, K, 4, brk_ids, names, region_extremes=True)
        assert f3.tobytes() == f4.tobytes()
        # behind the region calls when both are on
        posteriors.add_region_calls(res, regions, {'log_prob': -rng.uniform(size=R), 'log_prob_call': -rng.uniform(size=R), 'n_differ': rng.randint(0, 5, size=R)})
        f5, _ = restarts._pack(res, N, M, K, 4, brk_ids, names, region_names=regions, region_calls=True)
        f6, _ = restarts._pack(res, N, M, K, 4, brk_ids, names, region_names=regions, region_calls=True, region_extremes=True)
        assert f6[:len(f5)].tobytes() == f5.tobytes() and f6[len(f5):].tobytes() == f2[len(f0):].tobytes()
    off = restarts.gather_result_records(full, e, ps, M, names, region_names=regions)
    on = restarts.gather_result_records(full, e, ps, M, names, region_names=regions, region_extremes=True)
    for i, res in on.items():
        assert sorted(set(res) - {'region_cn_extremes'}) == sorted(off[i]) and 'region_cn_extremes' not in off[i]
        for k in posteriors.EXTREME_ARRAYS:
            assert np.array_equal(res['region_cn_extremes'][k], full[i]['region_cn_extremes'][k]), k
        for k in off[i]:
            if isinstance(off[i][k], np.ndarray):
                assert np.array_equal(off[i][k], res[k], equal_nan=True), k
    # the entry points refuse the option without regions before any fit
    from remixt_amd.analysis import pipeline
    small = synthetic.make_experiment(20, num_clones=3, max_copy_number=3, num_chains=2, seed=0)
    sp = synthetic.make_init_params(small, 2, 3)
    with pytest.raises(ValueError, match='needs cn_regions'):
        pipeline.fit_restarts(small, dict(enumerate(sp)), {'cn_region_extremes': True})
    with pytest.raises(ValueError, match='needs cn_regions'):
        pipeline.fit(small, sp[0], {'cn_region_extremes': True})
    with pytest.raises(ValueError, match='needs cn_regions'):
        restarts.fit_restarts_distributed(small, sp, 3, cn_region_extremes=True)


def test_no_extremes_without_the_kernel():
    from oracle import oracle
    from tests import helpers as H
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError):
        mo.region_cn_extremes([(1, 2)])
    with pytest.raises(NotImplementedError):
        mo.region_clone_extremes([(1, 2)])
