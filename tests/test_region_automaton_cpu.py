"""Host side of the region automata (remixt_amd/posteriors.py) and their numpy twin, without a GPU: the twin against
brute-force path enumeration, the three builders against direct counting, reverse_automaton, symbols_from and level_mask,
batch_event_runs / batch_event_run_of / batch_region_automaton over a stand-in batch that answers region_automaton_raw from
the twin, and the query tuple, symbol, header, kernel text and methods."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest

from remixt_amd import posteriors, queries, restarts
from tests import automaton_twin, region_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_delta(rng, Q, A):
    return rng.randint(0, Q, size=(Q, A))


def _permutation_delta(rng, Q, A):
    return np.stack([rng.permutation(Q) for _ in range(A)], axis=1)


def test_twin_against_enumeration():
    """6 segments, 4 states, two chains (4 + 2 segments), a skipped segment: a many-to-one delta, a permutation delta and Q = 1."""
    rng = np.random.RandomState(41)
    N, S = 6, 4
    f = rng.normal(scale=2., size=(N, S))
    T = rng.normal(scale=2., size=(N - 1, S, S))
    T[3] = 0.      # (the adjacency across the chain end, as log_transmat holds it)
    twin = region_twin.RegionTwin(f, T, [0, 4], [3, 5])
    unreachable = 0
    for name, Q, A, delta in (('many-to-one', 5, 3, None), ('permutation', 4, 3, _permutation_delta(rng, 4, 3)), ('one state', 1, 2, np.zeros((1, 2), dtype=int)),
                              ('collapse', 3, 2, np.array([[2, 2], [2, 2], [2, 2]]))):
        if delta is None:
            delta = _random_delta(rng, Q, A)
            delta[:, 0] = delta[0, 0]           # symbol 0 sends every state to one
        sym = rng.randint(0, A, size=(N, S))
        for start in (0, Q - 1):
            for constrain in (None, np.array([1, 0, 1, 1, 1, 1], dtype=bool), np.array([1, 1, 1, 0, 1, 0], dtype=bool), np.zeros(N, dtype=bool)):
                for (a, b), (c0, c1) in [((0, 3), (0, 4)), ((1, 2), (0, 4)), ((0, 0), (0, 4)), ((3, 3), (0, 4)), ((1, 3), (0, 4)), ((4, 5), (4, 6)), ((5, 5), (4, 6))]:
                    want = automaton_twin.brute_force(f[c0:c1], T[c0:c1 - 1], a - c0, b - c0, sym[c0:c1], delta, start,
                                                      None if constrain is None else constrain[c0:c1])
                    got = automaton_twin.logfinal(twin, a, b, sym, delta, start, constrain)
                    assert got.shape == (Q,)
                    assert np.array_equal(got == -np.inf, want == -np.inf), (name, a, b, got, want)
                    assert (np.abs(np.exp(got) - np.exp(want)) <= 1e-12).all(), (name, a, b, got, want)
                    assert abs(np.exp(got).sum() - 1) <= 1e-12
                    unreachable += int((want == -np.inf).sum())
                    if constrain is not None and not constrain.any():
                        assert got[start] == pytest.approx(0., abs=1e-12)        # nothing is read: the automaton stays where it started
    assert unreachable >= 50


def _strings(A, L):
    return itertools.product(range(A), repeat=L)


def test_builders_against_direct_counting():
    for bins in (1, 2, 3, 8):
        au = posteriors.automaton_runs(bins)
        assert au.delta.shape == (2 * bins, 2) and au.delta.dtype == np.uint8 and au.start == 0 and au.alphabet == 2 and len(au.value) == 2 * bins
        for L in range(0, 9):
            for s in _strings(2, L):
                runs = sum(1 for i in range(L) if s[i] == 1 and (i == 0 or s[i - 1] == 0))
                for order in (s, s[::-1]):          # reversal-symmetric: the reading order does not matter
                    assert au.value[automaton_twin.run_automaton(order, au.delta, au.start)] == min(runs, bins - 1), (bins, s)
    for k in (1, 2, 3, 15):
        au = posteriors.automaton_run_of(k)
        assert au.delta.shape == (k + 1, 2) and au.alphabet == 2
        for L in range(0, 9):
            for s in _strings(2, L):
                longest = max([0] + [len(r) for r in ''.join(map(str, s)).split('0')])
                for order in (s, s[::-1]):
                    assert (automaton_twin.run_automaton(order, au.delta, au.start) == k) == (longest >= k), (k, s)
    s = (1,) * 15
    assert automaton_twin.run_automaton(s, posteriors.automaton_run_of(15).delta, 0) == 15 and automaton_twin.run_automaton(s[:14], posteriors.automaton_run_of(15).delta, 0) == 14
    for bins in (1, 2, 4, 7):
        au = posteriors.automaton_switches(bins)
        assert au.delta.shape == (1 + 2 * bins, 3) and au.alphabet == 3 and au.delta.max() < 1 + 2 * bins
        for L in range(0, 7):
            for s in _strings(3, L):
                seen = [x for x in s if x != 0]
                switches = sum(1 for i in range(1, len(seen)) if seen[i] != seen[i - 1])
                for order in (s, s[::-1]):
                    assert au.value[automaton_twin.run_automaton(order, au.delta, au.start)] == min(switches, bins - 1), (bins, s)
    for bad in (lambda: posteriors.automaton_runs(0), lambda: posteriors.automaton_runs(9), lambda: posteriors.automaton_run_of(0),
                lambda: posteriors.automaton_run_of(16), lambda: posteriors.automaton_switches(0), lambda: posteriors.automaton_switches(8)):
        with pytest.raises(ValueError):
            bad()


def test_reverse_automaton():
    # left to right: a run of symbol 1, then at least one 0, then a run of symbol 2 -- "gain, then neutral, then loss", an ordered pattern
    # states: 0 nothing yet, 1 in the gain run, 2 neutral after it, 3 in the loss run (accepting), 4 dead
    delta = np.array([[0, 1, 4], [2, 1, 4], [2, 4, 3], [3, 3, 3], [4, 4, 4]])
    rev, acc = posteriors.reverse_automaton(delta, 0, [3])
    assert rev.delta.shape[0] <= 16 and rev.delta.shape[1] == 3 and rev.start == 0 and acc.dtype == bool and len(acc) == rev.delta.shape[0]
    hits = 0
    for L in range(0, 8):
        for s in _strings(3, L):
            want = automaton_twin.run_automaton(s, delta, 0) == 3
            assert bool(acc[automaton_twin.run_automaton(s[::-1], rev.delta, rev.start)]) == want, s
            hits += want
    assert hits > 100
    # a random automaton, accept as a boolean vector
    rng = np.random.RandomState(3)
    d2 = _random_delta(rng, 4, 2)
    flag = np.array([False, True, False, True])
    rev2, acc2 = posteriors.reverse_automaton(d2, 2, flag)
    for L in range(0, 9):
        for s in _strings(2, L):
            assert bool(acc2[automaton_twin.run_automaton(s[::-1], rev2.delta, rev2.start)]) == bool(flag[automaton_twin.run_automaton(s, d2, 2)])
    # "the sixth symbol from the left is 1" needs 2^6 states when read from the right
    Q = 8
    d3 = np.array([[min(q + 1, Q - 1)] * 2 for q in range(Q)])
    d3[5] = (7, 6)
    d3[6] = (6, 6)
    with pytest.raises(ValueError):
        posteriors.reverse_automaton(d3, 0, [6])


def _classes():
    """Two state classes, five states, three clones: the second class has one more copy of each allele in clone 2."""
    cn = np.array([[[1, 1], [1, 1], [1, 1]], [[1, 1], [2, 1], [1, 1]], [[1, 1], [1, 0], [2, 0]], [[1, 1], [0, 0], [0, 0]], [[1, 1], [3, 2], [2, 2]]])
    both = np.stack([cn, cn])
    both[1, :, 2, :] += 1
    return both


def test_symbols_from_and_level_mask():
    cn = _classes()
    masks, _ = posteriors.event_tables(cn)
    loh, hdel, sub = (masks[:, posteriors.MASK_NAMES.index(k)] != 0 for k in ('loh', 'hdel', 'subclonal'))
    sym = posteriors.symbols_from(cn, ['hdel', 'loh', sub])
    assert sym.dtype == np.int16 and sym.shape == cn.shape[:2]
    assert np.array_equal(sym, np.where(hdel, 1, np.where(loh, 2, np.where(sub, 3, 0))))         # the first part that holds
    assert np.array_equal(posteriors.symbols_from(cn, []), np.zeros(cn.shape[:2]))
    gain = posteriors.level_mask(cn, 'total', 1, 3, 99)
    assert gain.dtype == bool and np.array_equal(gain, cn[:, :, 1].sum(axis=-1) >= 3)
    assert np.array_equal(posteriors.level_mask(cn, 'minor', 'any', 0, 0), cn[:, :, 1:].min(axis=-1).max(axis=-1) == 0)
    assert np.array_equal(posteriors.symbols_from(cn, [gain, 'not_loh']), np.where(gain, 1, np.where(~loh, 2, 0)))
    for bad in (lambda: posteriors.symbols_from(cn, ['amplified']), lambda: posteriors.symbols_from(cn, [np.zeros((2, 4), dtype=bool)]),
                lambda: posteriors.symbols_from(cn, ['loh'] * 16), lambda: posteriors.level_mask(cn, 'total', 3, 0, 1),
                lambda: posteriors.level_mask(cn, 'depth', 1, 0, 1)):
        with pytest.raises(ValueError):
            bad()


class StandIn(object):
    """A batch that answers region_automaton_raw from the twin: 8 model segments, the fourth one inserted, chains [0, 4] and [5, 7]."""

    def __init__(self, nr=2):
        rng = np.random.RandomState(5)
        self.cn_classes = _classes()
        self.seg_class = np.array([0, 1, 0, 0, 1, 1, 0, 1])
        S = self.cn_classes.shape[1]
        self.fwd = np.array([0, 1, 2, 4, 5, 6, 7])
        self.orig = np.array([1, 1, 1, 0, 1, 1, 1, 1], dtype=bool)
        self.tel = np.array([0, 0, 0, 0, 1, 0, 0, 1])
        self.maps = (self.fwd, self.orig, self.tel)
        self.fT, self.twins = [], []
        for _ in range(nr):
            f = rng.normal(size=(8, S)); T = rng.normal(scale=1.5, size=(7, S, S))
            T[4] = 0.
            self.fT.append((f, T))
            self.twins.append(region_twin.RegionTwin(f, T, [0, 5], [4, 7]))
        self.calls = []

    def region_automaton_raw(self, r0, nr, q, symbols, delta, start, constrain=None):
        q, symbols, delta, start = np.asarray(q), np.asarray(symbols), np.asarray(delta), np.asarray(start)
        self.calls.append(len(q))
        assert symbols.shape[0] == 2 and symbols.shape[2] == 5 and delta.ndim == 3 and start.shape == (delta.shape[0],)
        out = np.zeros((nr, len(q), delta.shape[1]))
        for r in range(nr):
            for i, (a, b, si, ui) in enumerate(q):
                out[r, i] = automaton_twin.logfinal(self.twins[r0 + r], a, b, symbols[self.seg_class, si], delta[ui], start[ui], constrain)
        return out


def _enumerate_chain(b, r, c0, c1):
    """(paths, weights) of the chain of model segments c0 .. c1 of restart r."""
    f, T = b.fT[r]
    S = f.shape[1]
    paths = list(itertools.product(range(S), repeat=c1 - c0 + 1))
    w = np.array([np.exp(sum(f[c0 + i, p[i]] for i in range(len(p))) + sum(T[c0 + i, p[i], p[i + 1]] for i in range(len(p) - 1))) for p in paths])
    return paths, w / w.sum()


def test_event_runs_with_combine_counts():
    b = StandIn()
    cn = b.cn_classes
    event = posteriors.level_mask(cn, 'total', 2, 2, 2)
    ev_seg = event[b.seg_class]                        # (model segments, states)
    bins = 4
    regions = [(0, 6), (0, 3), (1, 2), (4, 6), (2, 5), (5, 5)]           # experiment segments; (0, 6) and (2, 5) span both chains
    out = posteriors.batch_event_runs(b, 0, 2, regions, *b.maps, event=event, bins=bins)
    assert b.calls == [8] and out['num_events'].shape == (2, len(regions), bins) and out['p_any'].shape == (2, len(regions))
    assert np.abs(out['num_events'].sum(axis=-1) - 1).max() <= 1e-12
    run3 = posteriors.batch_event_run_of(b, 0, 2, regions, *b.maps, event=event, k=2)
    assert run3['p_run'].shape == (2, len(regions))
    for r in range(2):
        chains = [(_enumerate_chain(b, r, 0, 4), 0), (_enumerate_chain(b, r, 5, 7), 5)]
        for i, (x, y) in enumerate(regions):
            A, B = b.fwd[x], b.fwd[y]
            pmf = np.zeros(bins)
            pmf[0] = 1.
            miss = 1.
            for (paths, w), c0 in chains:
                lo, hi = max(A, c0), min(B, c0 + len(paths[0]) - 1)
                if lo > hi:
                    continue
                piece = np.zeros(bins)
                has = 0.
                for p, wp in zip(paths, w):
                    s = [int(ev_seg[n, p[n - c0]]) for n in range(lo, hi + 1) if b.orig[n]]          # the inserted segment is not read
                    runs = sum(1 for j in range(len(s)) if s[j] and (j == 0 or not s[j - 1]))
                    piece[min(runs, bins - 1)] += wp
                    has += wp * (max([0] + [len(t) for t in ''.join(map(str, s)).split('0')]) >= 2)
                pmf = np.array([sum(pmf[u] * piece[v] for u in range(bins) for v in range(bins) if min(u + v, bins - 1) == k) for k in range(bins)])
                miss *= 1. - has
            assert np.abs(out['num_events'][r, i] - pmf).max() <= 1e-12, (r, i)
            assert abs(out['p_any'][r, i] - (1 - pmf[0])) <= 1e-12
            assert abs(run3['p_run'][r, i] - (1. - miss)) <= 1e-12, (r, i)
    # a mask name as the event
    named = posteriors.batch_event_runs(b, 0, 1, [(0, 3)], *b.maps, event='subclonal', bins=3)
    table = posteriors.batch_event_runs(b, 0, 1, [(0, 3)], *b.maps, event=posteriors.event_tables(cn)[0][:, 4] != 0, bins=3)
    assert np.array_equal(named['num_events'], table['num_events'])
    empty = posteriors.batch_event_runs(b, 0, 2, [], *b.maps, event='loh')
    assert empty['num_events'].shape == (2, 0, 8) and empty['p_any'].shape == (2, 0)
    with pytest.raises(ValueError):
        posteriors.batch_event_runs(b, 0, 1, [(0, 3)], *b.maps, event='loh', bins=9)
    with pytest.raises(ValueError):
        posteriors.batch_event_run_of(b, 0, 1, [(0, 3)], *b.maps, event='loh', k=16)


def test_batch_region_automaton():
    b = StandIn()
    cn = b.cn_classes
    au = posteriors.automaton_switches(3)
    sym = posteriors.symbols_from(cn, [posteriors.level_mask(cn, 'total', 1, 0, 2), posteriors.level_mask(cn, 'total', 1, 3, 99)])
    regions = [(0, 3), (4, 6), (2, 2)]
    accept = [i for i, v in enumerate(au.value) if v >= 1]
    out = posteriors.batch_region_automaton(b, 0, 2, regions, *b.maps, automaton=au, symbols=sym, accept=accept)
    assert out['log_final'].shape == (2, 3, 7) and out['final'].shape == (2, 3, 7) and out['p_accept'].shape == (2, 3) and b.calls == [3]
    for r in range(2):
        for i, (x, y) in enumerate(regions):
            want = automaton_twin.logfinal(b.twins[r], b.fwd[x], b.fwd[y], sym[b.seg_class], au.delta, au.start, b.orig)
            assert np.array_equal(out['log_final'][r, i], want)
            assert abs(out['p_accept'][r, i] - np.exp(want)[accept].sum()) <= 1e-15
    assert (out['p_accept'][:, 2] == 0).all()          # one segment cannot switch
    flag = np.zeros(7, dtype=bool)
    flag[accept] = True
    assert np.array_equal(posteriors.batch_region_automaton(b, 0, 2, regions, *b.maps, automaton=au, symbols=sym, accept=flag)['p_accept'], out['p_accept'])
    assert 'p_accept' not in posteriors.batch_region_automaton(b, 0, 1, regions, *b.maps, automaton=au, symbols=sym)
    # a region in two chains: the automaton's state does not cross a chain end
    with pytest.raises(ValueError, match=r'region 1 \(2, 5\)'):
        posteriors.batch_region_automaton(b, 0, 1, [(0, 1), (2, 5)], *b.maps, automaton=au, symbols=sym)
    for bad in (dict(automaton=au._replace(start=7)), dict(automaton=au._replace(delta=au.delta + 1)), dict(symbols=sym[:, :4]),
                dict(automaton=au._replace(delta=np.zeros((17, 2), dtype=int)))):
        with pytest.raises(ValueError):
            posteriors.batch_region_automaton(b, 0, 1, regions, *b.maps, **dict(dict(automaton=au, symbols=sym), **bad))
    none = posteriors.batch_region_automaton(b, 0, 2, [], *b.maps, automaton=au, symbols=sym, accept=accept)
    assert none['final'].shape == (2, 0, 7) and none['p_accept'].shape == (2, 0)


def test_query_entries():
    assert [e.name for e in queries.AUTOMATON_QUERIES] == ['region_automaton', 'event_runs', 'event_run_of']
    for e in queries.AUTOMATON_QUERIES:
        assert queries.BY_NAME[e.name] is e and e.needs == 'region_automaton_raw' and e not in queries.QUERIES and e not in queries.LATER_QUERIES
        assert e.doc and e.cn is None and not e.shared
    assert all(queries.BY_NAME[e.name] is e for e in queries.QUERIES + queries.LATER_QUERIES)
    assert len(queries.BY_NAME) == len(queries.QUERIES) + len(queries.LATER_QUERIES) + 3
    from remixt_amd import cn_model
    want = {'region_automaton': ['regions', 'automaton', 'symbols', 'accept'], 'event_runs': ['regions', 'event', 'bins'], 'event_run_of': ['regions', 'event', 'k']}
    for cls in (cn_model.BreakpointModel, restarts.RestartSet, restarts.RestartGroups, restarts.DatasetGroups):
        for name, params in want.items():
            method = getattr(cls, name)
            assert callable(method) and method.__doc__, (cls, name)
            assert [p for p in inspect.signature(method).parameters if p != 'self'][:len(params)] == params, (cls, name)
    assert 'FROM ITS LAST SEGMENT TO ITS FIRST' in cn_model.BreakpointModel.region_automaton.__doc__
    # a result along the restart axis: arrays are concatenated; one restart's entry loses the axis
    e = queries.BY_NAME['event_runs']
    parts = [{'num_events': np.full((n, 2, 8), n), 'p_any': np.full((n, 2), n)} for n in (1, 2)]
    joined = queries._join(parts, e.shared, e.extend, e.each)
    assert joined['num_events'].shape == (3, 2, 8) and joined['p_any'].shape == (3, 2)
    assert queries._only(e, parts[0])['num_events'].shape == (2, 8)


# the kernel names of the parent commit, in id order: rmx_num_kernels() = 32 with k_restart_overlap, rmx_num_profile_ids() = 33
_PARENT_KERNELS = [
    'k_state_tables', 'k_seg_const', 'k_framelogprob', 'k_fb', 'k_marginals<true>', 'k_marginals<false>', 'k_update_outlier_total',
    'k_update_outlier_allele', 'k_update_allele_swap', 'k_brk_lut', 'k_pairwise', 'k_brk_update', 'k_elbo_seg', 'k_elbo_final',
    'k_ell_list', 'k_ell_final', 'k_ell_full', 'k_viterbi', 'k_backtrace', 'other', 'k_sample_cn', 'k_posterior_summary', 'k_region_prob',
    'k_region_counts', 'k_call_prob', 'k_region_moments', 'k_region_extent', 'k_region_span', 'k_region_pattern', 'k_region_decode',
    'k_region_extremes']


def test_declared_and_bound():
    from remixt_amd import _lib, bpmodel
    assert 'rmx_region_automaton' in _lib.SYMBOLS and len(_lib.SYMBOLS['rmx_region_automaton'][1]) == 14
    with open(os.path.join(ROOT, 'include', 'remixt_amd.h')) as fh:
        text = re.sub(r'\s+', ' ', fh.read())
    assert ('int rmx_region_automaton(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t nsym, const int16_t *symbols, '
            'int32_t nauto, int32_t Q, int32_t A, const uint8_t *delta, const int32_t *start, const uint8_t *constrain, double *logp_out);') in text
    assert 'DESIGN 4.23' in text and 'FROM ITS LAST SEGMENT TO ITS FIRST' in text and 'NOT READ' in text and '1e-308 below the total' in text
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_api.hip')) as fh:
        api = fh.read()
    # the kernel has no id: the three name lists are the parent's, 31 + 1 + 1 names
    names = re.findall(r'"([^"]*)"', re.search(r'kKernelNames\[KID_COUNT\] = \{(.*?)\};', api, re.S).group(1))
    assert names == _PARENT_KERNELS
    assert re.findall(r'"([^"]*)"', re.search(r'kPairKernelNames\[KID_ALL - KID_COUNT\] = \{(.*?)\};', api, re.S).group(1)) == ['k_restart_overlap']
    assert re.findall(r'"([^"]*)"', re.search(r'kLaterKernelNames\[KID_PROFILE_ALL - KID_ALL\] = \{(.*?)\};', api, re.S).group(1)) == ['k_region_conditional']
    assert len(names) + 1 == 32 and 'k_region_automaton' not in re.findall(r'"([^"]*)"', api)
    assert 'int rmx_region_automaton(' in api and re.search(r'run_queries\(b, r0, nr, nq, queries, \(int\)Q, KID_NONE, "region_automaton', api)
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_host.h')) as fh:
        host = fh.read()
    assert 'inline bool automaton_shape_ok(int32_t nauto, int32_t Q, int32_t A)' in host
    assert 'inline int64_t check_automata(int32_t nauto, int32_t Q, int32_t A, const uint8_t *delta, const int32_t *start)' in host
    assert 'inline int64_t check_symbols(int64_t C, int64_t nsym, int64_t S, int32_t A, const int16_t *symbols)' in host
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_kernels.h')) as fh:
        kern = fh.read()
    # (the slices of the earlier kernels' tests stay what they were: behind k_restart_overlap, in front of k_region_kbest's section)
    assert kern.index('void k_restart_overlap(') < kern.index('void k_region_automaton(') < kern.index('// Region alternatives:') < kern.index('void k_region_kbest(')
    body = kern[kern.index('void k_region_automaton('):kern.index('// Region alternatives:')]
    assert body.count('__builtin_amdgcn_mfma_f64_16x16x4f64(') == 1 and 'atomicAdd' not in body and 'asm' not in body
    assert body.count('atomicOr(&flags[r]') == 1 and body.count('atomic') == 1 and 'DESIGN 4.23' in kern
    assert hasattr(bpmodel.RemixtBatch, 'region_automaton_raw') and hasattr(bpmodel.RemixtModel, 'region_automaton')


def test_no_region_automaton_without_the_kernel():
    from oracle import oracle
    from tests import helpers as H
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError):
        mo.event_runs([(1, 4)], 'loh')
    with pytest.raises(NotImplementedError):
        mo.event_run_of([(1, 4)], 'hdel', 2)
    with pytest.raises(NotImplementedError):
        mo.region_automaton([(1, 4)], posteriors.automaton_runs(2), np.zeros((1, 1), dtype=int))
