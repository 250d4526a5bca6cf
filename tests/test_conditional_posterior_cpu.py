"""CPU: the conditional posteriors given a region event off the device -- the numpy twin against the enumeration
of every path of small chains, posteriors.evidence_shift, the mapping of regions and windows onto model segments with
inserted segments, posteriors.conditional_unpack, and the declarations: the header, _lib.SYMBOLS, the profile accessors
over all three id ranges, and rmx_num_kernels / rmx_kernel_name as they were."""
import os
import re

import numpy as np
import pytest

from remixt_amd import posteriors, restarts
from tests import conditional_twin, region_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chain(N, S, seed):
    rng = np.random.RandomState(seed)
    return rng.normal(0., 2., (N, S)), rng.normal(0., 2., (N - 1, S, S))


def _twin(f, T):
    N = f.shape[0]
    return region_twin.RegionTwin(f, T, np.array([0]), np.array([N - 1]))


N, S = 5, 3
MASK = np.array([[1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0], [0, 1, 1]], dtype=bool)
LABEL = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
ALL = np.ones(N, dtype=bool)
SOME = np.array([1, 0, 1, 0, 1], dtype=bool)


@pytest.mark.parametrize('a,b,mask,label,constrain', [
    (1, 3, MASK, None, ALL),               # mask
    (1, 3, None, LABEL, ALL),              # label
    (1, 3, MASK, LABEL, ALL),              # both
    (0, 4, MASK, None, SOME),              # segments inside the run that the mask does not bind
    (1, 3, MASK, LABEL, SOME),
    (2, 2, MASK, None, ALL),               # one segment
    (2, 2, None, LABEL, ALL),              # one segment and a label: no adjacency, nothing binds
    (0, 1, MASK, LABEL, ALL),              # evidence at the chain's first segment
    (3, 4, MASK, LABEL, None),             # evidence at its last; constrain None binds everywhere
    (0, 4, MASK, LABEL, ALL),              # the whole chain
    (1, 3, None, None, ALL),               # no constraint: the unconditional marginals
])
def test_twin_against_enumeration(a, b, mask, label, constrain):
    f, T = _chain(N, S, 3 * a + b)
    want, want_lp = conditional_twin.brute_force(f, T, a, b, mask, label, constrain)
    assert np.isfinite(want_lp) and np.allclose(want.sum(axis=1), 1., atol=1e-14)
    got, lp = conditional_twin.conditional(_twin(f, T), a, b, 0, N - 1, mask, label, constrain)
    assert abs(lp - want_lp) <= 1e-13 and np.abs(got - want).max() <= 1e-14, (lp, want_lp, np.abs(got - want).max())
    # log P(E) is region_twin's, and a narrower window is a slice of the wide one
    assert abs(lp - region_twin.brute_force(f, T, a, b, mask, label, constrain)) <= 1e-13
    lo, hi = max(a - 1, 0), min(b + 1, N - 1)
    part, lp2 = conditional_twin.conditional(_twin(f, T), a, b, lo, hi, mask, label, constrain)
    assert lp2 == lp and np.array_equal(part, got[lo:hi + 1])
    if mask is None and label is None:
        none, _ = conditional_twin.brute_force(f, T, 0, 0)
        assert abs(lp) <= 1e-15 and np.abs(got - none).max() <= 1e-14
    if mask is not None:
        bound = np.array([a <= n <= b and (constrain is None or constrain[n]) for n in range(N)])
        assert (got[bound][~mask[bound]] == 0).all()


def test_twin_impossible_event():
    f, T = _chain(N, S, 11)
    mask = MASK.copy(); mask[2] = False
    got, lp = conditional_twin.conditional(_twin(f, T), 1, 3, 0, N - 1, mask, None, ALL)
    want, want_lp = conditional_twin.brute_force(f, T, 1, 3, mask, None, ALL)
    assert lp == -np.inf and want_lp == -np.inf and np.isnan(got).all() and np.isnan(want).all()
    # the same mask where segment 2 does not bind is possible
    got, lp = conditional_twin.conditional(_twin(f, T), 1, 3, 0, N - 1, mask, None, ~np.eye(N, dtype=bool)[2])
    assert np.isfinite(lp) and np.allclose(got.sum(axis=1), 1.)
    # labels that no transition keeps
    label = np.array([[0, 0, 0], [1, 1, 1]] * 2 + [[0, 0, 0]])
    got, lp = conditional_twin.conditional(_twin(f, T), 0, 4, 0, N - 1, None, label, ALL)
    assert lp == -np.inf and np.isnan(got).all()


def _summary(n, M, seed, inside=None):
    rng = np.random.RandomState(seed)
    s = {'total_cn_mean': rng.uniform(0, 4, (n, M)), 'total_cn_sd': rng.uniform(0, 1, (n, M)), 'expected_alleles_subclonal': rng.uniform(0, 2, n),
         'p_subclonal': rng.uniform(0, 1, n), 'p_loh': rng.uniform(0, 1, n), 'p_hdel': rng.uniform(0, 1, n), 'cn_posterior_max': rng.uniform(0, 1, n),
         'cn_mpm': rng.randint(0, 3, (n, M, 2))}
    if inside is not None:
        for k, v in s.items():
            s[k] = np.where(inside.reshape((n,) + (1,) * (v.ndim - 1)), v, -1 if k == 'cn_mpm' else np.nan)
    return s


def test_evidence_shift():
    n, M = 7, 3
    inside = np.array([0, 1, 1, 1, 1, 0, 0], dtype=bool)
    unc = dict(_summary(n, M, 0), cn_posterior_entropy=np.ones(n))
    cond = dict(_summary(n, M, 1, inside), log_evidence=-2.5)
    cond['cn_mpm'][2] = unc['cn_mpm'][2]
    sh = posteriors.evidence_shift(cond, unc)
    assert sh['log_evidence'] == -2.5 and 'cn_posterior_entropy' not in sh and 'cn_mpm' not in sh and 'ploidy_before' not in sh
    for k in ('total_cn_mean', 'total_cn_sd', 'expected_alleles_subclonal', 'p_subclonal', 'p_loh', 'p_hdel', 'cn_posterior_max'):
        assert np.array_equal(sh[k][inside], (cond[k] - unc[k])[inside]) and np.isnan(sh[k][~inside]).all(), k
    want = inside & np.any(cond['cn_mpm'] != unc['cn_mpm'], axis=(1, 2))
    assert np.array_equal(sh['cn_mpm_changed'], want) and not sh['cn_mpm_changed'][2] and not sh['cn_mpm_changed'][~inside].any()
    l = np.array([5., 1., 2., 0., 3., 7., 9.])
    sh = posteriors.evidence_shift(cond, unc, l)
    for name, s in (('ploidy_before', unc), ('ploidy_after', cond)):
        want = (s['total_cn_mean'][inside][:, 1:].sum(axis=1) * l[inside]).sum() / ((M - 1) * l[inside].sum())
        assert abs(sh[name] - want) <= 1e-15, name
    # evidence that cannot happen: nothing is inside
    none = dict(_summary(n, M, 1, np.zeros(n, dtype=bool)), log_evidence=-np.inf)
    sh = posteriors.evidence_shift(none, unc, l)
    assert np.isnan(sh['ploidy_after']) and np.isnan(sh['p_loh']).all() and not sh['cn_mpm_changed'].any()


# 9 experiment segments in chains [0, 3], [4, 8]; the model inserts a segment after experiment segments 1 and 5
FWD = np.array([0, 1, 3, 4, 5, 6, 8, 9, 10])
ORIG = np.array([1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1], dtype=bool)
TEL = np.array([0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1])


def test_window_and_region_mapping():
    cs, ce = posteriors.chains_from_telomeres(TEL)
    assert cs.tolist() == [0, 5] and ce.tolist() == [4, 10]
    regions = [(1, 2), (3, 5), (8, 8), (0, 8)]
    runs, windows, piece_region, constrain = posteriors.conditional_queries(regions, 'chain', FWD, ORIG, cs, ce)
    # (1, 2) holds the inserted segment 2; (3, 5) and (0, 8) span both chains: one piece each
    assert runs.tolist() == [[1, 3], [4, 4], [5, 6], [10, 10], [0, 4], [5, 10]] and piece_region.tolist() == [0, 1, 1, 2, 3, 3]
    assert windows.tolist() == [[0, 4], [0, 4], [5, 10], [5, 10], [0, 4], [5, 10]]
    assert np.array_equal(constrain, ORIG.astype(np.uint8)) and runs.dtype == np.int32 and windows.dtype == np.int32
    _, w1, _, _ = posteriors.conditional_queries(regions, 1, FWD, ORIG, cs, ce)
    assert w1.tolist() == [[0, 4], [3, 4], [5, 7], [9, 10], [0, 4], [5, 10]]      # cut at the chain's ends
    _, w0, _, _ = posteriors.conditional_queries(regions, 0, FWD, ORIG, cs, ce)
    assert np.array_equal(w0, runs)
    for bad in ('arm', -1, 1.5, (1, 2)):
        with pytest.raises(ValueError):
            posteriors.conditional_queries(regions, bad, FWD, ORIG, cs, ce)
    with pytest.raises(ValueError):
        posteriors.conditional_queries([(2, 1)], 'chain', FWD, ORIG, cs, ce)
    runs, windows, piece_region, _ = posteriors.conditional_queries([], 'chain', FWD, ORIG, cs, ce)
    assert runs.shape == (0, 2) and windows.shape == (0, 2) and len(piece_region) == 0


def test_conditional_event():
    cn = np.zeros((2, 4, 3, 2), dtype=int)
    cn[:, :, 0] = 1
    cn[:, 1, 1:] = (1, 0); cn[:, 2, 1:] = (2, 1); cn[:, 3, 1] = (1, 1)
    masks, labels, mi, li = posteriors.conditional_event(('loh', 'total'), cn)
    em, el = posteriors.event_tables(cn)
    assert np.array_equal(masks, em) and np.array_equal(labels, el) and (mi, li) == posteriors.parse_event(('loh', 'total'))
    assert posteriors.conditional_event('hdel', cn)[2:] == (posteriors.MASK_NAMES.index('hdel'), -1)
    table = np.array([[1, 0, 0, 1], [0, 0, 1, 0]], dtype=bool)
    masks, labels, mi, li = posteriors.conditional_event(table, cn)
    assert masks.shape == (2, 1, 4) and masks.dtype == np.uint8 and np.array_equal(masks[:, 0], table) and labels is None and (mi, li) == (0, -1)
    with pytest.raises(ValueError):
        posteriors.conditional_event(table[:, :3], cn)
    with pytest.raises(ValueError):
        posteriors.conditional_event('nothing', cn)


def test_conditional_unpack():
    rng = np.random.RandomState(5)
    C_, S_, M = 2, 6, 3
    cn_classes = rng.randint(0, 3, (C_, S_, M, 2))
    seg_class = np.array([0, 1, 0, 1, 0, 0, 1, 0, 1, 0, 1])
    weights, layout = posteriors.feature_matrix(cn_classes)
    Q = layout['Q']
    cs, ce = posteriors.chains_from_telomeres(TEL)
    regions = [(1, 2), (3, 5)]
    runs, windows, piece_region, _ = posteriors.conditional_queries(regions, 1, FWD, ORIG, cs, ce)
    assert windows.tolist() == [[0, 4], [3, 4], [5, 7]]
    nslot = 5
    cond = rng.dirichlet(np.ones(S_), (3, nslot))                      # a conditional row per (piece, slot)
    out = np.full((3, nslot, Q + 3), np.nan)
    for p in range(3):
        L = windows[p, 1] - windows[p, 0] + 1
        cls = seg_class[windows[p, 0]:windows[p, 1] + 1]
        out[p, :L, :Q] = np.einsum('ks,ksq->kq', cond[p, :L], weights[cls])
        out[p, :L, Q], out[p, :L, Q + 1], out[p, :L, Q + 2] = cond[p, :L].max(axis=1), cond[p, :L].argmax(axis=1), cond[p, :L, 1]
    logp = np.array([-1., -0.5, -2.])
    res = posteriors.conditional_unpack(logp, out, windows, piece_region, 2, layout, cn_classes, seg_class, FWD, True)
    assert len(res) == 2 and res[0]['log_evidence'] == -1. and res[1]['log_evidence'] == -2.5
    assert set(res[0]) == set(posteriors.CONDITIONAL_ARRAYS) | {'log_evidence', 'cn_posterior_prob'}
    # region 0: model segments 0 .. 4 are experiment segments 0 .. 3 (model segment 2 is inserted and dropped)
    r0 = res[0]
    assert r0['p_loh'].shape == (9,) and r0['total_cn_mean'].shape == (9, M) and r0['cn_mpm'].shape == (9, M, 2)
    assert np.isfinite(r0['p_loh'][:4]).all() and np.isnan(r0['p_loh'][4:]).all() and (r0['cn_mpm'][4:] == -1).all()
    for e, n in enumerate(FWD[:4]):
        assert r0['p_loh'][e] == out[0, n, layout['loh']] and r0['cn_posterior_prob'][e] == cond[0, n, 1]
        assert np.array_equal(r0['cn_mpm'][e], cn_classes[seg_class[n], cond[0, n].argmax()])
    # region 1: a piece per chain, each with its own window
    r1 = res[1]
    inside = np.isfinite(r1['cn_posterior_max'])
    assert inside.tolist() == [False, False, True, True, True, True, False, False, False]      # model 3, 4 | 5, 6 (7 is inserted)
    assert r1['cn_posterior_max'][2] == cond[1, 0].max() and r1['cn_posterior_max'][4] == cond[2, 0].max()
    assert 'cn_posterior_prob' not in posteriors.conditional_unpack(logp, out, windows, piece_region, 2, layout, cn_classes, seg_class, FWD, False)[0]
    # an impossible piece: -inf evidence, NaN in its window
    out[1] = np.nan
    res = posteriors.conditional_unpack(np.array([-1., -np.inf, -2.]), out, windows, piece_region, 2, layout, cn_classes, seg_class, FWD, True)
    assert res[1]['log_evidence'] == -np.inf and np.isnan(res[1]['p_hdel'][2:4]).all() and np.isfinite(res[1]['p_hdel'][4:6]).all()
    assert (res[1]['cn_mpm'][2:4] == -1).all()


def test_declared_and_bound():
    from remixt_amd import _lib, bpmodel, cn_model
    assert 'rmx_region_conditional' in _lib.SYMBOLS and len(_lib.SYMBOLS['rmx_region_conditional'][1]) == 17
    assert 'rmx_num_profile_ids' in _lib.SYMBOLS and 'rmx_profile_name' in _lib.SYMBOLS
    with open(os.path.join(ROOT, 'include', 'remixt_amd.h')) as fh:
        text = re.sub(r'\s+', ' ', fh.read())
    assert ('int rmx_region_conditional(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, const int32_t *windows, '
            'int32_t nslot, int32_t nmask, const uint8_t *masks, int32_t nlabel, const int16_t *labels, const uint8_t *constrain, int32_t Q, '
            'const double *weights, const int16_t *states, double *logp_out, double *out);') in text
    assert 'DESIGN 4.20' in text and 'const char *rmx_profile_name(int32_t profile_id);' in text and 'int rmx_num_profile_ids(void);' in text
    lib = _lib.load()
    # the two closed lists answer as before
    names = [lib.rmx_kernel_name(i).decode() for i in range(lib.rmx_num_kernels())]
    assert len(names) == 32 and names[0] == 'k_state_tables' and names[-2:] == ['k_region_extremes', 'k_restart_overlap']
    assert 'k_region_conditional' not in names and lib.rmx_kernel_name(len(names)).decode() == '' and lib.rmx_kernel_name(-1).decode() == ''
    # the profile accessors run over all three ranges
    ids = lib.rmx_num_profile_ids()
    pnames = [lib.rmx_profile_name(i).decode() for i in range(ids)]
    assert ids == len(names) + 1 and pnames[:len(names)] == names and pnames[-1] == 'k_region_conditional'
    assert len(set(pnames)) == len(pnames) and lib.rmx_profile_name(ids).decode() == '' and lib.rmx_profile_name(-1).decode() == ''
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_host.h')) as fh:
        host = fh.read()
    assert 'inline int64_t check_conditional(' in host and 'inline size_t conditional_pairs(' in host
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_kernels.h')) as fh:
        kern = fh.read()
    start = kern.index('void k_region_conditional(')
    assert start > kern.index('void k_region_decode(')
    body = kern[kern.index('int rgc_emit('):kern.index('// Restart overlap:')]
    for piece in ('rgn_tabs(', 'rgn_adj(', 'rgn_compact(', 'rgn_D_exp(', 'rgn_take_sum(', 'rgn_block_sum('):
        assert piece in body, piece
    assert 'atomicAdd' not in body and body.count('atomicOr(&flags[r]') == 1 and 'mfma' not in body
    assert hasattr(bpmodel.RemixtBatch, 'region_conditional_raw') and hasattr(bpmodel.RemixtModel, 'region_conditional')
    for cls in (cn_model.BreakpointModel, restarts.RestartSet, restarts.RestartGroups, restarts.DatasetGroups):
        assert hasattr(cls, 'conditional_summary'), cls
