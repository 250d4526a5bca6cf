"""Host side of the region sums (remixt_amd/posteriors.py) and their numpy twin, without a GPU: the twin against brute-force
path enumeration, quantise_lengths' bracket, occupancy_at_least against direct enumeration, batch_region_sums /
batch_event_occupancy and the four class levels over a stand-in batch that answers region_sums_raw from the twin, and the
query tuple, symbol, header, kernel text and build dependencies."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest

from remixt_amd import posteriors, queries, restarts
from tests import region_twin, sums_twin
from tests.test_region_automaton_cpu import _PARENT_KERNELS, _classes, _enumerate_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_twin_against_enumeration():
    """6 segments, 4 states, two chains (4 + 2 segments); weights with zeros and one that saturates (also past 32 bits);
    1, 2, 5 and 64 bins."""
    rng = np.random.RandomState(43)
    N, S = 6, 4
    f = rng.normal(scale=2., size=(N, S))
    T = rng.normal(scale=2., size=(N - 1, S, S))
    T[3] = 0.      # (the adjacency across the chain end, as log_transmat holds it)
    twin = region_twin.RegionTwin(f, T, [0, 4], [3, 5])
    assert posteriors.sums_max_bins(S) == 64                   # (the bins below are bins the device call takes at this state count)
    unreachable = saturated = 0
    for name, level in (('mask', rng.randint(0, 2, size=(N, S))), ('levels', rng.randint(0, 4, size=(N, S))), ('high', rng.randint(0, 2, size=(N, S)) * 32767)):
        for weights in ([1, 1, 1, 1, 1, 1], [2, 0, 3, 1, 0, 5], [1, 0, 70, 2, 2 ** 31 - 1, 1], [0, 0, 0, 0, 0, 0]):
            for bins in (1, 2, 5, 64):
                for (a, b), (c0, c1) in [((0, 3), (0, 4)), ((1, 2), (0, 4)), ((0, 0), (0, 4)), ((3, 3), (0, 4)), ((1, 3), (0, 4)), ((4, 5), (4, 6)), ((5, 5), (4, 6))]:
                    w = weights[a:b + 1]
                    want = sums_twin.brute_force(f[c0:c1], T[c0:c1 - 1], a - c0, b - c0, level[c0:c1], w, bins)
                    got = sums_twin.logsums(twin, a, b, level, w, bins)
                    assert got.shape == (bins,)
                    assert np.array_equal(got == -np.inf, want == -np.inf), (name, weights, bins, a, b, got, want)
                    assert (np.abs(np.exp(got) - np.exp(want)) <= 1e-12).all(), (name, weights, bins, a, b, got, want)
                    assert abs(np.exp(got).sum() - 1) <= 1e-12
                    unreachable += int((want == -np.inf).sum())
                    saturated += int(bins > 2 and want[-1] > -np.inf and max(w) >= 70)
                    if not any(w):
                        assert got[0] == pytest.approx(0., abs=1e-12)        # nothing counts: the sum is 0
    assert unreachable >= 50 and saturated >= 10


def test_max_bins_table():
    assert [posteriors.sums_max_bins(S) for S in (1, 165, 304, 305, 355, 457, 608, 609, 1024, 1025, 0, -3)] == [64, 64, 64, 32, 32, 32, 32, 16, 16, 0, 0, 0]


def test_quantise_lengths_bracket():
    rng = np.random.RandomState(7)
    for trial in range(200):
        n = rng.randint(1, 12)
        l = rng.uniform(0.1, 50., size=n) if trial % 2 else rng.randint(1, 2000, size=n).astype(float)
        l[rng.rand(n) < 0.2] = 0.
        bins, vmax = int(rng.choice([8, 16, 64])), int(rng.choice([1, 1, 3]))
        unit, wf, wc, exact = posteriors.quantise_lengths(l, bins, vmax)
        assert wf.dtype == np.int64 and wc.dtype == np.int64 and unit > 0
        assert (wf * unit <= l * (1 + 1e-14)).all() and (l <= wc * unit * (1 + 1e-14)).all() and (wc - wf <= 1).all() and (wf >= 0).all()
        assert ((l == 0) <= (wc == 0)).all()
        assert exact == bool(np.array_equal(wf, wc))
        pos = int((l > 0).sum())
        cap = (bins - 1) // vmax
        if pos <= cap:
            assert wc.sum() * vmax <= bins - 1                       # nothing saturates
            if pos:                                                  # and no smaller unit would do: a unit a hair below breaks the rule
                _, _, wc2, _ = posteriors.quantise_lengths(l, bins, vmax, unit=unit * (1 - 1e-9))
                assert wc2.sum() * vmax > bins - 1
        else:                                                        # the saturating fallback: the floor side fits
            assert wf.sum() * vmax <= bins - 1 < wc.sum() * vmax
        # the bracket for every choice of levels
        for _ in range(5):
            lev = rng.randint(0, vmax + 1, size=n)
            assert unit * (wf * lev).sum() <= (l * lev).sum() * (1 + 1e-14) and (l * lev).sum() <= unit * (wc * lev).sum() * (1 + 1e-14)
    # gridded lengths are exact where the grid is the smallest unit that fits (9 units in 10 bins), and under a unit that divides them
    unit, wf, wc, exact = posteriors.quantise_lengths([3000., 1000., 0., 5000.], 10)
    assert exact and np.array_equal(wf, [3, 1, 0, 5]) and abs(unit - 1000.) <= 1e-9
    unit, wf, wc, exact = posteriors.quantise_lengths([3000., 1000., 0., 5000.], 16)       # 15 units: 625 each, no longer the grid
    assert not exact and abs(unit - 625.) <= 1e-9 and np.array_equal(wc, [5, 2, 0, 8]) and np.array_equal(wf, [4, 1, 0, 8])
    unit, wf, wc, exact = posteriors.quantise_lengths([3000., 1000., 5000.], 64, unit=500.)
    assert exact and np.array_equal(wc, [6, 2, 10]) and unit == 500.
    unit, wf, wc, exact = posteriors.quantise_lengths([3000., 1000., 5000.], 64, unit=700.)
    assert not exact and np.array_equal(wf, [4, 1, 7]) and np.array_equal(wc, [5, 2, 8])
    # the fallback: 20 segments do not fit 8 bins one unit each
    l = np.arange(1., 21.)
    unit, wf, wc, exact = posteriors.quantise_lengths(l, 8)
    assert not exact and wf.sum() <= 7 < wc.sum() and (wc >= 1).all()
    assert posteriors.quantise_lengths([0., 0.], 8) == (1., pytest.approx([0, 0]), pytest.approx([0, 0]), True)
    assert posteriors.quantise_lengths([], 8)[3] is True
    for bad in (lambda: posteriors.quantise_lengths([1., -1.], 8), lambda: posteriors.quantise_lengths([1.], 0), lambda: posteriors.quantise_lengths([1.], 8, unit=0.),
                lambda: posteriors.quantise_lengths([np.nan], 8)):
        with pytest.raises(ValueError):
            bad()


class StandIn(object):
    """A batch that answers region_sums_raw from the twin: 8 model segments, the fourth one inserted, chains [0, 4] and [5, 7]."""
    num_segments, num_cn_states = 8, 5

    def __init__(self, nr=2):
        rng = np.random.RandomState(5)
        self.cn_classes = _classes()
        self.seg_class = np.array([0, 1, 0, 0, 1, 1, 0, 1])
        S = self.cn_classes.shape[1]
        self.fwd = np.array([0, 1, 2, 4, 5, 6, 7])
        self.orig = np.array([1, 1, 1, 0, 1, 1, 1, 1], dtype=bool)
        self.tel = np.array([0, 0, 0, 0, 1, 0, 0, 1])
        self.maps = (self.fwd, self.orig, self.tel)
        self.l1 = np.array([3000., 1000., 2500., 0., 500., 4000., 1500., 700.])
        self.fT, self.twins = [], []
        for _ in range(nr):
            f = rng.normal(size=(8, S)); T = rng.normal(scale=1.5, size=(7, S, S))
            T[4] = 0.
            self.fT.append((f, T))
            self.twins.append(region_twin.RegionTwin(f, T, [0, 5], [4, 7]))
        self.calls = []

    def region_sums_raw(self, r0, nr, q, levels, weights, bins):
        q, levels, weights = np.asarray(q), np.asarray(levels), np.asarray(weights)
        self.calls.append(len(q))
        assert levels.shape[0] == 2 and levels.shape[2] == 5 and weights.ndim == 1 and weights.dtype == np.int32 and (weights >= 0).all()
        out = np.zeros((nr, len(q), bins))
        for r in range(nr):
            for i, (a, b, li, o) in enumerate(q):
                assert 0 <= o and o + (b - a) < len(weights)
                out[r, i] = sums_twin.logsums(self.twins[r0 + r], a, b, levels[self.seg_class, li], [int(x) for x in weights[o:o + b - a + 1]], bins)
        return out


def _region_sum_pmf(b, r, region, level_seg, w, bins=None):
    """The distribution of sum_n w[n] level(c_n) over the model segments of an experiment region by enumerating both chains:
    a dict value -> probability (bins None), or the pmf with the last bin absorbing."""
    A, B = b.fwd[region[0]], b.fwd[region[1]]
    dist = {0: 1.}
    for c0, c1 in ((0, 4), (5, 7)):
        lo, hi = max(A, c0), min(B, c1)
        if lo > hi:
            continue
        paths, pw = _enumerate_chain(b, r, c0, c1)
        piece = {}
        for p, wp in zip(paths, pw):
            v = sum(w[n] * level_seg[n, p[n - c0]] for n in range(lo, hi + 1))
            piece[v] = piece.get(v, 0.) + wp
        new = {}
        for u, pu in dist.items():
            for v, pv in piece.items():
                new[u + v] = new.get(u + v, 0.) + pu * pv
        dist = new
    if bins is None:
        return dist
    pmf = np.zeros(bins)
    for v, p in dist.items():
        pmf[min(int(v), bins - 1)] += p
    return pmf


REGIONS = [(0, 6), (0, 3), (1, 2), (4, 6), (2, 5), (5, 5)]           # experiment segments; (0, 6) and (2, 5) span both chains


def test_batch_region_sums():
    b = StandIn()
    cn = b.cn_classes
    levels = cn[:, :, 2].sum(axis=-1)                   # the total of clone 2: the two classes differ
    w = np.array([1, 2, 0, 3, 1, 1, 4, 0])
    for bins in (5, 64):
        b.calls = []
        out = posteriors.batch_region_sums(b, 0, 2, REGIONS, *b.maps, levels=levels, weights=w, bins=bins)
        assert b.calls == [8] and out['bins'] == bins and out['pmf'].shape == (2, len(REGIONS), bins)
        for r in range(2):
            for i, reg in enumerate(REGIONS):
                want = _region_sum_pmf(b, r, reg, levels[b.seg_class], w, bins)
                assert np.abs(out['pmf'][r, i] - want).max() <= 1e-12, (bins, r, i)
                assert abs(out['mean'][r, i] - (want * np.arange(bins)).sum()) <= 1e-10 and abs(out['p_saturated'][r, i] - want[-1]) <= 1e-12
    assert posteriors.batch_region_sums(b, 0, 1, [(0, 1)], *b.maps, levels=levels, weights=w)['bins'] == 64      # (5 states: the most bins)
    none = posteriors.batch_region_sums(b, 0, 2, [], *b.maps, levels=levels, weights=w, bins=4)
    assert none['pmf'].shape == (2, 0, 4)
    for bad in (dict(levels=levels[:, :4]), dict(levels=-levels), dict(weights=w[:7]), dict(weights=-w), dict(weights=w.astype(float)), dict(bins=0), dict(bins=65)):
        with pytest.raises(ValueError):
            posteriors.batch_region_sums(b, 0, 1, REGIONS, *b.maps, **dict(dict(levels=levels, weights=w, bins=8), **bad))


def test_event_occupancy_and_at_least():
    b = StandIn()
    cn = b.cn_classes
    event = posteriors.level_mask(cn, 'total', 2, 2, 2)
    lev_seg = event[b.seg_class].astype(int)
    # by segments: exact, the inserted segment weighs nothing
    out = posteriors.batch_event_occupancy(b, 0, 2, REGIONS, *b.maps, b.l1, event, weights='segments', bins=16)
    assert b.calls == [16]                               # one call holds the floor and the ceil queries of the 8 pieces
    assert out['bins'] == 16 and out['exact'].all() and (out['unit'] == 1).all() and np.array_equal(out['length'], [7, 4, 2, 3, 4, 1])
    assert np.array_equal(out['pmf_floor'], out['pmf_ceil'])
    for r in range(2):
        for i, reg in enumerate(REGIONS):
            want = _region_sum_pmf(b, r, reg, lev_seg, b.orig.astype(int), 16)
            assert np.abs(out['pmf_floor'][r, i] - want).max() <= 1e-12
            assert abs(out['mean_floor'][r, i] - (want * np.arange(16)).sum()) <= 1e-10
    assert (out['p_saturated'] <= 1e-15).all()
    lo, hi = posteriors.occupancy_at_least(out, 0.5)
    assert lo.shape == (2, len(REGIONS)) and np.array_equal(lo, hi)
    for r in range(2):
        for i, reg in enumerate(REGIONS):
            dist = _region_sum_pmf(b, r, reg, lev_seg, b.orig.astype(int))
            assert abs(lo[r, i] - sum(p for v, p in dist.items() if v >= 0.5 * out['length'][i])) <= 1e-12
    # by length: the lengths are multiples of 100, but 64 bins do not hold every region at that unit: a bracket around the truth
    b.calls = []
    out = posteriors.batch_event_occupancy(b, 0, 2, REGIONS, *b.maps, b.l1, event, weights='length', bins=64)
    assert b.calls == [16] and out['pmf_floor'].shape == (2, len(REGIONS), 64)
    lens = np.where(b.orig, b.l1, 0.)
    assert np.allclose(out['length'], [13200., 7000., 3500., 6200., 8500., 1500.])
    assert out['exact'][5] and out['unit'][5] <= 1500. / 63 * (1 + 1e-12)              # one segment: any unit that divides it
    assert out['exact'][2] and abs(out['unit'][2] - 500. / 9) <= 1e-9                     # 1000 and 2500: 18 + 45 units of 500 / 9
    for fraction in (0.1, 0.5, 0.9, 1.0):
        lo, hi = posteriors.occupancy_at_least(out, fraction)
        for r in range(2):
            for i, reg in enumerate(REGIONS):
                dist = _region_sum_pmf(b, r, reg, lev_seg, lens)
                truth = sum(p for v, p in dist.items() if v >= fraction * out['length'][i] * (1 - 1e-12))
                assert lo[r, i] - 1e-12 <= truth <= hi[r, i] + 1e-12, (fraction, r, i, lo[r, i], truth, hi[r, i])
                if out['exact'][i]:
                    assert abs(lo[r, i] - hi[r, i]) <= 1e-15
        assert (lo <= hi + 1e-15).all()
    for r in range(2):
        for i, reg in enumerate(REGIONS):
            dist = _region_sum_pmf(b, r, reg, lev_seg, lens)
            mean = sum(v * p for v, p in dist.items())
            assert out['mean_floor'][r, i] - 1e-8 <= mean <= out['mean_ceil'][r, i] + 1e-8
    # a given unit that is the grid: exact everywhere, and the pmf is the truth's
    exact = posteriors.batch_event_occupancy(b, 0, 2, REGIONS[1:], *b.maps, b.l1, event, weights='length', bins=64, unit=500.)
    assert exact['exact'].tolist() == [True, True, False, True, True]                    # (700 is no multiple of 500)
    want = _region_sum_pmf(b, 1, REGIONS[1], lev_seg, lens / 500., 64)
    assert np.abs(exact['pmf_floor'][1, 0] - want).max() <= 1e-12 and np.array_equal(exact['pmf_floor'][:, 0], exact['pmf_ceil'][:, 0])
    # a unit too small: the last bin takes what does not fit, and a threshold past it is not resolved
    tight = posteriors.batch_event_occupancy(b, 0, 2, REGIONS[:1], *b.maps, b.l1, event, weights='length', bins=8, unit=1000.)
    assert (tight['p_saturated'] > 0).all() and np.isinf(tight['mean_ceil']).all() and np.isfinite(tight['mean_floor']).all()
    # a threshold that rounding leaves an ulp above an integer is that integer: 0.2 * 3 / 0.1 = 6.000000000000001 in doubles
    snap = dict(tight, length=np.array([3.]), unit=np.array([0.1]), bins=16, pmf_floor=np.eye(16)[None, 6:7], pmf_ceil=np.eye(16)[None, 6:7])
    assert 0.2 * 3. / 0.1 > 6 and posteriors.occupancy_at_least(snap, 0.2)[0][0, 0] == 1 and posteriors.occupancy_at_least(snap, 0.2)[1][0, 0] == 1
    lo, hi = posteriors.occupancy_at_least(tight, 0.9)                                   # 11.88 units: past 7
    assert (lo == 0).all() and np.array_equal(hi, tight['p_saturated'])
    # a copy-number feature: the copies the segments carry between them
    feat = posteriors.batch_event_occupancy(b, 0, 1, [(0, 2)], *b.maps, b.l1, ('total', 2), weights='segments', bins=32)
    want = _region_sum_pmf(b, 0, (0, 2), cn[:, :, 2].sum(axis=-1)[b.seg_class], b.orig.astype(int), 32)
    assert np.abs(feat['pmf_floor'][0, 0] - want).max() <= 1e-12
    named = posteriors.batch_event_occupancy(b, 0, 1, [(0, 3)], *b.maps, b.l1, 'subclonal', weights='segments', bins=8)
    table = posteriors.batch_event_occupancy(b, 0, 1, [(0, 3)], *b.maps, b.l1, posteriors.event_tables(cn)[0][:, 4] != 0, weights='segments', bins=8)
    assert np.array_equal(named['pmf_floor'], table['pmf_floor'])
    empty = posteriors.batch_event_occupancy(b, 0, 2, [], *b.maps, b.l1, 'loh')
    assert empty['pmf_floor'].shape == (2, 0, 64) and empty['unit'].shape == (0,)
    for bad in (dict(event='amplified'), dict(event=('total', 3)), dict(event=('depth', 1)), dict(weights='area'), dict(bins=65), dict(unit=-1.)):
        with pytest.raises(ValueError):
            posteriors.batch_event_occupancy(b, 0, 1, REGIONS, *b.maps, b.l1, **dict(dict(event='loh', weights='length', bins=8), **bad))


class _Model(object):
    """What the class levels need of a model: its batch, restart, maps and lengths."""

    def __init__(self, b, r):
        self._batch, self._r = b, r
        self.seg_fwd_remap, self.seg_is_original, self.is_telomere, self.l1 = b.fwd, b.orig, b.tel, b.l1


def test_query_entries_and_the_four_class_levels():
    assert [e.name for e in queries.SUM_QUERIES] == ['region_sums', 'event_occupancy']
    for e in queries.SUM_QUERIES:
        assert queries.entry(e.name) is e and e.needs == 'region_sums_raw' and e.lacks == 'has no region sums' and e.shared == ('bins', 'unit', 'length', 'exact')
        assert e.name not in queries.BY_NAME and e not in queries.ALL_QUERIES and e not in queries.ENTROPY_QUERIES and e.doc and e.cn is None
    from remixt_amd import cn_model
    want = {'region_sums': ['regions', 'levels', 'weights', 'bins'], 'event_occupancy': ['regions', 'event', 'weights', 'bins', 'unit']}
    for cls in (cn_model.BreakpointModel, restarts.RestartSet, restarts.RestartGroups, restarts.DatasetGroups):
        for name, params in want.items():
            method = getattr(cls, name)
            assert callable(method) and method.__doc__, (cls, name)
            assert [p for p in inspect.signature(method).parameters if p != 'self'] == params, (cls, name)
    for text in (cn_model.BreakpointModel.event_occupancy.__doc__, posteriors.batch_event_occupancy.__doc__):
        assert 'EXACT' in text and 'RIGOROUS BRACKET' in text and 'loose bracket' in text
    # the generic bodies over the stand-in batch: one restart loses the axis, a set keeps it, groups are joined, shared keys stay
    b = StandIn()
    e = queries.entry('event_occupancy')
    args = dict(regions=REGIONS, event='subclonal', weights='length', bins=32, unit=None)
    direct = posteriors.batch_event_occupancy(b, 0, 2, REGIONS, *b.maps, b.l1, 'subclonal', weights='length', bins=32)
    one = queries._only(e, e.call(queries.Restarts(b, 1, 1, [_Model(b, 1)]), **args))
    assert one['pmf_ceil'].shape == (len(REGIONS), 32) and np.array_equal(one['pmf_ceil'], direct['pmf_ceil'][1]) and one['bins'] == 32
    assert np.array_equal(one['unit'], direct['unit']) and one['exact'].shape == (len(REGIONS),)
    whole = e.call(queries.Restarts(b, 0, 2, [_Model(b, 0), _Model(b, 1)]), **args)
    parts = [e.call(queries.Restarts(b, r, 1, [_Model(b, r)]), **args) for r in (0, 1)]
    joined = queries._join(parts, e.shared, e.extend, e.each)
    assert sorted(joined) == sorted(whole) and all(np.array_equal(joined[k], whole[k]) for k in whole)
    assert joined['pmf_floor'].shape == (2, len(REGIONS), 32) and joined['length'].shape == (len(REGIONS),)
    s = queries.entry('region_sums')
    w = np.array([1, 2, 0, 3, 1, 1, 4, 0])
    got = queries._only(s, s.call(queries.Restarts(b, 0, 1, [_Model(b, 0)]), regions=REGIONS, levels=b.cn_classes[:, :, 1].sum(axis=-1), weights=w, bins=16))
    assert got['pmf'].shape == (len(REGIONS), 16) and got['bins'] == 16 and abs(got['pmf'].sum(axis=-1) - 1).max() <= 1e-12


def test_declared_and_bound():
    from remixt_amd import _lib, bpmodel
    import __graft_entry__ as entry
    assert 'rmx_region_sums' in _lib.SYMBOLS and len(_lib.SYMBOLS['rmx_region_sums'][1]) == 11
    with open(os.path.join(ROOT, 'include', 'remixt_amd.h')) as fh:
        text = re.sub(r'\s+', ' ', fh.read())
    assert ('int rmx_region_sums(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t nlevel, const int16_t *levels, '
            'int32_t nwt, const int32_t *weights, int32_t nbins, double *logp_out);') in text
    assert 'DESIGN 4.25' in text and 'ONE SCALE CARRIES ALL COLUMNS' in text and '1e-308 below the total' in text and 'There is no constrain vector' in text
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_api.hip')) as fh:
        api = fh.read()
    # the kernel has no id: the three name lists are the parent's
    names = re.findall(r'"([^"]*)"', re.search(r'kKernelNames\[KID_COUNT\] = \{(.*?)\};', api, re.S).group(1))
    assert names == _PARENT_KERNELS and 'k_region_sums' not in re.findall(r'"([^"]*)"', api)
    assert 'int rmx_region_sums(' in api and re.search(r'run_queries\(b, r0, nr, nq, queries, \(int\)nbins, KID_NONE, "region_sums', api)
    assert api.index('#include "rmx_kernels.h"') < api.index('#include "rmx_region_sums.h"')
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_host.h')) as fh:
        host = fh.read()
    for decl in ('inline int32_t sums_max_bins(int32_t S)', 'inline int64_t sums_lds_bytes(int32_t S, int32_t nbins)',
                 'inline int32_t sum_increment(int32_t w, int32_t level, int32_t nbins)', 'inline int64_t check_weights(int64_t nwt, const int32_t *weights)',
                 'inline int64_t check_sum_spans(int32_t nq, const int32_t *queries, int64_t nwt)'):
        assert decl in host, decl
    path = os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_region_sums.h')
    assert path in [os.path.abspath(p) for p in entry.HIP_DEPS]
    with open(path) as fh:
        kern = fh.read()
    body = kern[kern.index('void k_region_sums('):]
    assert body.count('__builtin_amdgcn_mfma_f64_16x16x4f64(') == 1 and 'atomicAdd' not in body and 'asm' not in body
    assert body.count('atomicOr(&flags[r]') == 1 and body.count('atomic') == 1 and 'DESIGN 4.25' in kern
    for shared in ('rgn_adj(', 'rgn_compact(', 'rgn_D_exp(', 'rgn_take_sum(', 'rgn_block_sum('):
        assert shared in body, shared
    assert hasattr(bpmodel.RemixtBatch, 'region_sums_raw') and hasattr(bpmodel.RemixtModel, 'region_sums')


def test_no_region_sums_without_the_kernel():
    from oracle import oracle
    from tests import helpers as H
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError, match='has no region sums'):
        mo.event_occupancy([(1, 4)], 'loh')
    with pytest.raises(NotImplementedError, match='has no region sums'):
        mo.region_sums([(1, 4)], np.zeros((1, 1), dtype=int), np.zeros(30, dtype=int))
