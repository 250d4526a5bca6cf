"""Host side of the locus joints (remixt_amd/posteriors.py) and their numpy twin, without a GPU: the twin against
brute-force path enumeration, joint_summary on hand-made tables, the level tables, locus_queries, batch_locus_joint and
batch_locus_dependence over a stand-in batch that answers locus_joint_raw from the twin, and the symbol, header, kernel id
lists, host rules and methods."""
import os
import re

import numpy as np
import pytest

from remixt_amd import posteriors, queries, restarts
from tests import locus_twin, region_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_twin_against_enumeration():
    """Chains of 4 - 5 segments with 3 - 4 states: a = t, adjacent loci, the whole chain, different row and column tables, an
    empty level, and levels past the table."""
    rng = np.random.RandomState(23)
    empty = 0
    for N, S in ((5, 3), (4, 4)):
        f = rng.normal(scale=2., size=(N, S))
        T = rng.normal(scale=2., size=(N - 1, S, S))
        twin = region_twin.RegionTwin(f, T, [0], [N - 1])
        row = rng.randint(0, 3, size=(N, S))
        col = rng.randint(0, 4, size=(N, S))
        row[0] = np.where(row[0] == 1, 2, row[0])        # level 1 is empty at segment 0
        col[N - 1] = np.arange(S) % 2 + 2                # levels 0 and 1 are empty at the last segment
        for a, t in [(0, 0), (2, 2), (N - 1, N - 1), (0, 1), (1, 2), (N - 2, N - 1), (0, N - 1), (1, N - 1), (0, 2)]:
            for lr, lc, nrow, ncol in ((row, col, 3, 4), (col, row, 4, 3), (row, row, 3, 3), (col, col, 2, 2)):
                want = locus_twin.brute_force(f, T, a, t, nrow, ncol, lr, lc)
                got = locus_twin.logtable(twin, a, t, nrow, ncol, lr, lc)
                assert got.shape == (nrow, ncol)
                assert np.array_equal(got == -np.inf, want == -np.inf), (N, S, a, t, got, want)
                assert (np.abs(np.exp(got) - np.exp(want)) <= 1e-12).all(), (N, S, a, t, got, want)
                empty += int((want == -np.inf).sum())
                covered = (lr[a].max() < nrow) and (lc[t].max() < ncol)
                total = np.exp(got).sum()
                assert abs(total - 1) <= 1e-12 if covered else total < 1 - 1e-6, (a, t, nrow, ncol, total)
                if a == t and lr is lc:
                    off = got[~np.eye(nrow, ncol, dtype=bool)]
                    assert (off == -np.inf).all()        # one segment, one table: the diagonal is the level marginal
        # the marginals of a table that covers every state are the one-segment tables of the two loci
        g = np.exp(locus_twin.logtable(twin, 0, N - 1, 3, 4, row, col))
        ma = np.exp(np.diag(locus_twin.logtable(twin, 0, 0, 3, 3, row, row)))
        mb = np.exp(np.diag(locus_twin.logtable(twin, N - 1, N - 1, 4, 4, col, col)))
        assert np.abs(g.sum(axis=1) - ma).max() <= 1e-12 and np.abs(g.sum(axis=0) - mb).max() <= 1e-12
    assert empty >= 20


def test_twin_with_two_chains():
    rng = np.random.RandomState(6)
    S = 3
    f = rng.normal(size=(7, S)); T = rng.normal(size=(6, S, S))
    T[3] = 0.      # (the adjacency across the chain end, as log_transmat holds it)
    both = region_twin.RegionTwin(f, T, [0, 4], [3, 6])
    lv = rng.randint(0, 3, size=(7, S))
    assert np.abs(np.exp(locus_twin.logtable(both, 1, 3, 3, 3, lv, lv)) - np.exp(locus_twin.brute_force(f[:4], T[:3], 1, 3, 3, 3, lv[:4], lv[:4]))).max() <= 1e-12
    assert np.abs(np.exp(locus_twin.logtable(both, 4, 6, 3, 3, lv, lv)) - np.exp(locus_twin.brute_force(f[4:], T[4:], 0, 2, 3, 3, lv[4:], lv[4:]))).max() <= 1e-12


def test_joint_summary():
    pa, pb = np.array([0.2, 0.5, 0.3, 0.]), np.array([0.1, 0.1, 0.4, 0.4])
    with np.errstate(divide='ignore'):
        s = posteriors.joint_summary(np.log(np.stack([pa[:, None] * pb[None, :], np.diag(pa), np.outer([0, 1., 0, 0], pb), np.diag([0, 0, 0.25, 0.75])])), first_level=2)
    assert set(posteriors.JOINT_ARRAYS) <= set(s) and s['joint'].shape == (4, 4, 4) and s['difference_pmf'].shape == (4, 7)
    # an independent product: no information, no correlation
    assert abs(s['mutual_information'][0]) <= 1e-15 and abs(s['correlation'][0]) <= 1e-14
    assert np.abs(s['marginal_a'][0] - pa).max() <= 1e-15 and np.abs(s['marginal_b'][0] - pb).max() <= 1e-15
    assert abs(s['p_equal'][0] - (pa * pb).sum()) <= 1e-15 and abs(s['p_equal'][0] + s['p_a_higher'][0] + s['p_b_higher'][0] - 1) <= 1e-15
    assert abs(s['mean_difference'][0] - ((pa * np.arange(4)).sum() - (pb * np.arange(4)).sum())) <= 1e-14
    assert abs(s['difference_pmf'][0].sum() - 1) <= 1e-15 and abs(s['difference_pmf'][0][3] - s['p_equal'][0]) <= 1e-16
    assert abs(s['difference_pmf'][0][:3].sum() - s['p_b_higher'][0]) <= 1e-15 and abs(s['difference_pmf'][0][0] - pa[0] * pb[3]) <= 1e-16
    # a diagonal table: equal for sure, and knowing one is knowing the other
    entropy = -(pa[pa > 0] * np.log(pa[pa > 0])).sum()
    assert s['p_equal'][1] == 1 and s['p_a_higher'][1] == 0 and abs(s['mutual_information'][1] - entropy) <= 1e-15 and abs(s['correlation'][1] - 1) <= 1e-14
    assert s['difference_pmf'][1][3] == 1 and s['mean_difference'][1] == 0
    # a degenerate marginal: no correlation to speak of, no information
    assert np.isnan(s['correlation'][2]) and s['mutual_information'][2] == 0 and not np.isnan(s['correlation'][:2]).any()
    # saturation: the mass with either level in the last bin
    assert abs(s['p_saturated'][0] - (pa[3] + pb[3] - pa[3] * pb[3])) <= 1e-15 and s['p_saturated'][1] == 0 and abs(s['p_saturated'][3] - 0.75) <= 1e-15
    assert abs(s['p_saturated'][2] - 0.4) <= 1e-15
    # mutual information is clipped at 0 and at most the smaller marginal entropy
    rng = np.random.RandomState(1)
    J = rng.dirichlet(np.ones(25), size=50).reshape(50, 5, 5)
    r = posteriors.joint_summary(np.log(J))
    H = lambda p: -(np.where(p > 0, p * np.log(np.where(p > 0, p, 1.)), 0.)).sum(axis=-1)
    assert (r['mutual_information'] >= 0).all() and (r['mutual_information'] <= np.minimum(H(r['marginal_a']), H(r['marginal_b'])) + 1e-12).all()
    assert (np.abs(r['correlation']) <= 1).all()
    # cells so small that the product of their marginals is 0 in double: the information stays finite and below the entropy
    with np.errstate(divide='ignore'):
        tiny = posteriors.joint_summary(np.log(np.array([[1 - 1e-9, 0., 0.], [0., 1e-9, 0.], [0., 0., 1e-200]])))
    assert 0 < tiny['mutual_information'] <= H(tiny['marginal_a']) * (1 + 1e-12) and np.isfinite(tiny['correlation'])
    # a table with a NaN (a slot outside the chain) gives NaN, not an error
    bad = posteriors.joint_summary(np.full((2, 3, 3), np.nan))
    assert np.isnan(bad['mutual_information']).all() and np.isnan(bad['correlation']).all() and np.isnan(bad['p_equal']).all()
    with pytest.raises(ValueError):
        posteriors.joint_summary(np.zeros((3, 4)))


def _classes():
    """Two state classes, five states, three clones: the second class has one more copy of each allele in clone 2."""
    cn = np.array([[[1, 1], [1, 1], [1, 1]], [[1, 1], [2, 1], [1, 1]], [[1, 1], [1, 0], [2, 0]], [[1, 1], [0, 0], [0, 0]], [[1, 1], [3, 2], [2, 2]]])
    both = np.stack([cn, cn])
    both[1, :, 2, :] += 1
    return both


def test_locus_level_tables():
    cn = _classes()
    C, S, M, _ = cn.shape
    for bins, first in ((8, 0), (3, 1), (1, 0)):
        levels, names = posteriors.locus_level_tables(cn, bins, first)
        assert levels.dtype == np.int16 and levels.shape == (C, 3 * M + 6, S) and levels.flags['C_CONTIGUOUS'] and levels.min() >= 0
        assert names == ['peak_%s_%s' % (q, c) for q in posteriors.LEVEL_QUANTITIES for c in (1, 2, 'any')] + list(posteriors.MASK_NAMES)
        ref, ref_names = posteriors.level_tables(cn, bins, first)
        assert np.array_equal(levels[:, :3 * M], ref[:, :3 * M]) and names[:3 * M] == ref_names[:3 * M]
        masks, _ = posteriors.event_tables(cn)
        assert np.array_equal(levels[:, 3 * M:], masks) and set(np.unique(levels[:, 3 * M:])) <= {0, 1}
        tot2 = cn[:, :, 2, :].sum(axis=-1)
        assert np.array_equal(levels[:, names.index('peak_total_2')], np.clip(tot2 - first, 0, bins - 1))
    assert posteriors.locus_feature_name(('major', 'any'), M) == 'peak_major_any' and posteriors.locus_feature_name('loh', M) == 'loh'
    for bad in (('total', 3), ('total', 0), ('depth', 1), 'amplified', 7):
        with pytest.raises(ValueError):
            posteriors.locus_feature_name(bad, M)


def test_locus_queries():
    fwd = np.array([0, 1, 2, 4, 5, 6, 7])                # model segment 3 is inserted
    cs, ce = np.array([0, 5]), np.array([4, 7])
    segs, swapped, cross = posteriors.locus_queries([(0, 3), (3, 0), (2, 2), (1, 5), (6, 4), (4, 3), (6, 5)], fwd, cs, ce)
    assert segs.dtype == np.int32 and segs.tolist() == [[0, 4], [0, 4], [2, 2], [1, 6], [5, 7], [4, 5], [6, 7]]
    assert swapped.tolist() == [False, True, False, False, True, True, True]
    assert cross.tolist() == [False, False, False, True, False, True, False]
    e = posteriors.locus_queries(np.zeros((0, 2), dtype=int), fwd, cs, ce)
    assert e[0].shape == (0, 2) and len(e[1]) == 0 and len(e[2]) == 0
    for bad in ([(0, 7)], [(-1, 2)]):
        with pytest.raises(ValueError):
            posteriors.locus_queries(bad, fwd, cs, ce)


class StandIn(object):
    """A batch that answers locus_joint_raw from the twin: 8 model segments, the fourth one inserted, chains [0, 4] and [5, 7]."""

    def __init__(self, nr=2):
        rng = np.random.RandomState(5)
        self.cn_classes = _classes()
        self.seg_class = np.array([0, 1, 0, 0, 1, 1, 0, 1])
        S = self.cn_classes.shape[1]
        self.fwd = np.array([0, 1, 2, 4, 5, 6, 7])
        self.orig = np.array([1, 1, 1, 0, 1, 1, 1, 1], dtype=bool)
        self.tel = np.array([0, 0, 0, 0, 1, 0, 0, 1])
        self.maps = (self.fwd, self.orig, self.tel)
        self.twins = []
        for _ in range(nr):
            f = rng.normal(size=(8, S)); T = rng.normal(scale=1.5, size=(7, S, S))
            T[4] = 0.
            self.twins.append(region_twin.RegionTwin(f, T, [0, 5], [4, 7]))
        self.calls = []

    def table(self, r, a, t, levels, vr, vc, nrow, ncol):
        return locus_twin.logtable(self.twins[r], a, t, nrow, ncol, levels[self.seg_class, vr], levels[self.seg_class, vc])

    def locus_joint_raw(self, r0, nr, q, levels, nrow, ncol, nslot=0):
        q = np.asarray(q)
        self.calls.append((len(q), nslot))
        assert (q[:, 0] <= q[:, 1]).all() and (nslot == 0 or (q[:, 1] - q[:, 0] < nslot).all())
        out = np.full((nr, len(q)) + ((nslot,) if nslot else ()) + (nrow, ncol), np.nan)
        for r in range(nr):
            for i, (a, t, vr, vc) in enumerate(q):
                if nslot == 0:
                    out[r, i] = self.table(r0 + r, a, t, levels, vr, vc, nrow, ncol)
                else:
                    for k in range(t - a + 1):
                        out[r, i, k] = self.table(r0 + r, t - k, t, levels, vr, vc, nrow, ncol)
        return out


def test_batch_locus_joint():
    b = StandIn()
    pairs = [(0, 3), (3, 0), (2, 2), (1, 5), (6, 4), (5, 1)]
    feature, other, bins = ('total', 1), ('major', 2), 6
    out = posteriors.batch_locus_joint(b, 0, 2, pairs, *b.maps, feature=feature, other=other, bins=bins)
    assert b.calls == [(4 + 2 * 2, 0)]       # one device call: four pairs of one chain, two times two marginals
    assert out['bins'] == bins and out['first_level'] == 0 and out['log_joint'].shape == (2, len(pairs), bins, bins)
    assert set(posteriors.JOINT_ARRAYS) <= set(out) and out['difference_pmf'].shape == (2, len(pairs), 2 * bins - 1)
    levels, names = posteriors.locus_level_tables(b.cn_classes, bins)
    fi, oi = names.index('peak_total_1'), names.index('peak_major_2')
    for r in range(2):
        # axis -2 is the pair's first locus with `feature`, whichever side of the other it lies on
        assert np.array_equal(out['log_joint'][r, 0], b.table(r, 0, 4, levels, fi, oi, bins, bins))
        assert np.array_equal(out['log_joint'][r, 1], b.table(r, 0, 4, levels, oi, fi, bins, bins).T)
        assert np.array_equal(out['log_joint'][r, 2], b.table(r, 2, 2, levels, fi, oi, bins, bins))
        # two chains: the outer product of the marginals, the first locus's along the rows
        assert np.array_equal(out['log_joint'][r, 4], b.table(r, 5, 7, levels, oi, fi, bins, bins).T)
        for k, (x, y) in ((3, (1, 6)), (5, (6, 1))):
            mx = np.diag(b.table(r, x, x, levels, fi, fi, bins, bins)); my = np.diag(b.table(r, y, y, levels, oi, oi, bins, bins))
            with np.errstate(invalid='ignore'):
                assert np.array_equal(out['log_joint'][r, k], mx[:, None] + my[None, :]), (r, k)
    # a swapped pair is the transpose when both loci read the same feature
    same = posteriors.batch_locus_joint(b, 0, 2, pairs, *b.maps, feature=feature, bins=bins)
    assert np.array_equal(same['log_joint'][:, 1], np.swapaxes(same['log_joint'][:, 0], -1, -2))
    assert np.abs(same['p_a_higher'][:, 1] - same['p_b_higher'][:, 0]).max() <= 1e-15      # (the same terms in another order)
    assert np.abs(same['joint'].sum(axis=(-2, -1)) - 1).max() <= 1e-12 and (same['mutual_information'][:, 3] <= 1e-12).all()
    assert (same['mutual_information'][:, 0] > 1e-4).all()
    # pair 4 = (6, 4) lies in one chain (model 7, 5); a mask feature against a level
    mixed = posteriors.batch_locus_joint(b, 1, 1, [(6, 4)], *b.maps, feature='loh', other=('total', 'any'), bins=4, first_level=1)
    lv4, n4 = posteriors.locus_level_tables(b.cn_classes, 4, 1)
    assert mixed['first_level'] == 1 and np.array_equal(mixed['log_joint'][0, 0], b.table(1, 5, 7, lv4, n4.index('peak_total_any'), n4.index('loh'), 4, 4).T)
    assert (mixed['log_joint'][0, 0, 2:] == -np.inf).all() and abs(mixed['joint'].sum() - 1) <= 1e-12
    none = posteriors.batch_locus_joint(b, 0, 2, [], *b.maps)
    assert none['log_joint'].shape == (2, 0, 8, 8) and none['p_equal'].shape == (2, 0)
    for bad in (dict(bins=0), dict(bins=17), dict(feature=('total', 3)), dict(other='gain')):
        with pytest.raises(ValueError):
            posteriors.batch_locus_joint(b, 0, 1, pairs, *b.maps, **bad)


def test_batch_locus_dependence():
    b = StandIn()
    anchors, W, bins = [3, 0, 6, 4], 3, 5
    out = posteriors.batch_locus_dependence(b, 0, 2, anchors, *b.maps, window=W, feature=('total', 1), other=('minor', 'any'), bins=bins)
    # experiment segments 0 .. 3 are one chain (model 0, 1, 2, 4: model 3 is inserted), 4 .. 6 the other
    assert out['segment'].tolist() == [[0, 1, 2, 3, -1, -1, -1], [-1, -1, -1, 0, 1, 2, 3], [-1, 4, 5, 6, -1, -1, -1], [-1, -1, -1, 4, 5, 6, -1]]
    # one profile call for the left halves, slots 0 .. 4 of anchor 3 (the inserted segment's slot among them); one pair call for the right
    assert b.calls == [(4, 5), (5, 0)]
    for k in posteriors.DEPENDENCE_ARRAYS:
        assert out[k].shape == (2, 4, 2 * W + 1) and np.isnan(out[k][:, out['segment'] < 0]).all(), k
        assert k == 'correlation' or not np.isnan(out[k][:, out['segment'] >= 0]).any(), k
    pairs = [(anchors[i], int(e)) for i in range(4) for e in out['segment'][i] if e >= 0]
    at = [(i, k) for i in range(4) for k in range(2 * W + 1) if out['segment'][i, k] >= 0]
    ref = posteriors.batch_locus_joint(b, 0, 2, pairs, *b.maps, feature=('total', 1), other=('minor', 'any'), bins=bins)
    for k in posteriors.DEPENDENCE_ARRAYS:
        got = np.stack([out[k][:, i, j] for i, j in at], axis=1)
        assert np.array_equal(got, ref[k], equal_nan=True), k
    # the anchor against itself with one feature on both sides: equal for sure
    own = posteriors.batch_locus_dependence(b, 0, 1, [2], *b.maps, window=1, bins=bins)
    assert abs(own['p_equal'][0, 0, 1] - 1) <= 1e-12 and own['segment'].tolist() == [[1, 2, 3]]
    empty = posteriors.batch_locus_dependence(b, 0, 2, [], *b.maps, window=2)
    assert empty['segment'].shape == (0, 5) and empty['p_equal'].shape == (2, 0, 5)
    with pytest.raises(ValueError):
        posteriors.batch_locus_dependence(b, 0, 1, [7], *b.maps)
    with pytest.raises(ValueError):
        posteriors.batch_locus_dependence(b, 0, 1, [1], *b.maps, window=-1)


def test_query_entries():
    assert [e.name for e in queries.LATER_QUERIES] == ['locus_joint', 'locus_dependence']
    for e in queries.LATER_QUERIES:
        assert queries.BY_NAME[e.name] is e and e.needs == 'locus_joint_raw' and e not in queries.QUERIES
    assert queries.BY_NAME['locus_joint'].shared == ('bins', 'first_level') and queries.BY_NAME['locus_dependence'].shared == ('bins', 'first_level', 'segment')
    assert all(queries.BY_NAME[e.name] is e for e in queries.QUERIES)
    # a result along the restart axis: the shared keys are the first part's, the arrays are concatenated; one restart's entry loses the axis
    parts = [{'bins': 4, 'first_level': 0, 'segment': np.arange(3)[None], 'p_equal': np.full((n, 1, 3), n)} for n in (1, 2)]
    e = queries.BY_NAME['locus_dependence']
    joined = queries._join(parts, e.shared, e.extend, e.each)
    assert joined['bins'] == 4 and joined['segment'].shape == (1, 3) and joined['p_equal'].shape == (3, 1, 3)
    one = queries._only(e, parts[0])
    assert one['segment'].shape == (1, 3) and one['p_equal'].shape == (1, 3) and one['bins'] == 4


# the kernel names of the parent commit, in id order: rmx_num_kernels() = 32 with k_restart_overlap, rmx_num_profile_ids() = 33
_PARENT_KERNELS = [
    'k_state_tables', 'k_seg_const', 'k_framelogprob', 'k_fb', 'k_marginals<true>', 'k_marginals<false>', 'k_update_outlier_total',
    'k_update_outlier_allele', 'k_update_allele_swap', 'k_brk_lut', 'k_pairwise', 'k_brk_update', 'k_elbo_seg', 'k_elbo_final',
    'k_ell_list', 'k_ell_final', 'k_ell_full', 'k_viterbi', 'k_backtrace', 'other', 'k_sample_cn', 'k_posterior_summary', 'k_region_prob',
    'k_region_counts', 'k_call_prob', 'k_region_moments', 'k_region_extent', 'k_region_span', 'k_region_pattern', 'k_region_decode',
    'k_region_extremes']


def test_declared_and_bound():
    from remixt_amd import _lib, bpmodel, cn_model
    assert 'rmx_locus_joint' in _lib.SYMBOLS and len(_lib.SYMBOLS['rmx_locus_joint'][1]) == 11
    with open(os.path.join(ROOT, 'include', 'remixt_amd.h')) as fh:
        text = re.sub(r'\s+', ' ', fh.read())
    assert ('int rmx_locus_joint(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t nlevel, const int16_t *levels, '
            'int32_t nrow, int32_t ncol, int32_t nslot, double *logp_out);') in text
    assert 'DESIGN 4.22' in text and '1e-308 below its column' in text
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_api.hip')) as fh:
        api = fh.read()
    # the kernel has no id: the three name lists are the parent's, 31 + 1 + 1 names
    names = re.findall(r'"([^"]*)"', re.search(r'kKernelNames\[KID_COUNT\] = \{(.*?)\};', api, re.S).group(1))
    assert names == _PARENT_KERNELS
    assert re.findall(r'"([^"]*)"', re.search(r'kPairKernelNames\[KID_ALL - KID_COUNT\] = \{(.*?)\};', api, re.S).group(1)) == ['k_restart_overlap']
    assert re.findall(r'"([^"]*)"', re.search(r'kLaterKernelNames\[KID_PROFILE_ALL - KID_ALL\] = \{(.*?)\};', api, re.S).group(1)) == ['k_region_conditional']
    assert len(names) + 1 == 32 and 'k_locus_joint' not in re.findall(r'"([^"]*)"', api)
    assert re.search(r'enum PairKernelId \{ KID_RESTART_OVERLAP = KID_COUNT, KID_ALL \};', api)
    assert re.search(r'enum LaterKernelId \{ KID_REGION_CONDITIONAL = KID_ALL, KID_PROFILE_ALL \};', api)
    assert 'int rmx_locus_joint(' in api and 'KID_NONE' in api
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_host.h')) as fh:
        host = fh.read()
    assert 'inline bool locus_shape_ok(int32_t nrow, int32_t ncol, int32_t nslot)' in host
    assert 'inline int64_t check_locus_lengths(int32_t nq, const int32_t *queries, int32_t nslot' in host
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_kernels.h')) as fh:
        kern = fh.read()
    assert kern.index('void k_call_prob(') < kern.index('void k_locus_joint(') < kern.index('int rgc_emit(')
    body = kern[kern.index('void k_locus_joint('):kern.index('// Region conditionals:')]
    assert body.count('__builtin_amdgcn_mfma_f64_16x16x4f64(') == 1 and 'atomicAdd' not in body and 'asm' not in body
    assert body.count('atomicOr(&flags[r]') == 1 and 'DESIGN 4.22' in kern
    assert hasattr(bpmodel.RemixtBatch, 'locus_joint_raw') and hasattr(bpmodel.RemixtModel, 'locus_joint')
    for cls in (cn_model.BreakpointModel, restarts.RestartSet, restarts.RestartGroups, restarts.DatasetGroups):
        for name in ('locus_joint', 'locus_dependence'):
            assert callable(getattr(cls, name)) and getattr(cls, name).__doc__, (cls, name)


def test_no_locus_joint_without_the_kernel():
    from oracle import oracle
    from tests import helpers as H
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError):
        mo.locus_joint([(1, 2)])
    with pytest.raises(NotImplementedError):
        mo.locus_dependence([3])
