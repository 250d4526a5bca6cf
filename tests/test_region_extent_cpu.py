"""Host side of the region event extents (remixt_amd/posteriors.py) and their numpy twin, without a GPU: the twin and the
restated right-walk recursion against brute-force path enumeration, extent_queries / extent_summary / batch_event_extents
against a batch answered by the twin, the distributed record with and without the section, the config checks, the
declarations."""
import numpy as np
import pytest

from remixt_amd import defaults, posteriors, restarts, synthetic
from tests import extent_twin, region_twin
from tests.test_cn_samples_records_cpu import _fake_result


def _small_chain(seed=5):
    rng = np.random.RandomState(seed)
    N, S = 6, 4
    f = rng.normal(scale=2., size=(N, S))
    T = rng.normal(scale=2., size=(N - 1, S, S))
    mask = rng.uniform(size=(N, S)) < 0.6
    mask[:, 0] = True                                   # (no segment without an allowed state)
    label = np.array([[0, 1, 0, 1], [0, 0, 1, 1]])[np.arange(N) % 2]      # (two state classes; both labels occur in each)
    constrain = np.ones(N, dtype=bool); constrain[3] = False
    return f, T, mask, label, constrain


# mask, label, both and neither
_EVENTS = [(True, False), (False, True), (True, True), (False, False)]


def _enumerated(f, T, n0, wl, wr, mask, label, constrain):
    N = len(f)
    out = np.full(wl + wr + 1, -np.inf)
    for k in range(wl + wr + 1):
        n = n0 - wl + k
        if 0 <= n < N:
            out[k] = region_twin.brute_force(f, T, min(n, n0), max(n, n0), mask, label, constrain)
    return out


@pytest.mark.parametrize('n0', [0, 2, 5])
def test_twin_against_enumeration(n0):
    f, T, mask, label, constrain = _small_chain()
    twin = region_twin.RegionTwin(f, T, [0], [5])
    worst = 0.
    for use_mask, use_label in _EVENTS:
        mk, lb = (mask if use_mask else None), (label if use_label else None)
        got = extent_twin.extent(twin, n0, 6, 6, mk, lb, constrain)
        want = _enumerated(f, T, n0, 6, 6, mk, lb, constrain)
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        # outside the chain: -inf on both sides of it
        assert np.isneginf(got[:6 - n0]).all() and np.isneginf(got[6 + (5 - n0) + 1:]).all() and np.isfinite(got[6 - n0:12 - n0]).all()
        err = np.abs(np.exp(got) - np.exp(want))
        worst = max(worst, err.max())
        assert (err <= 1e-12).all(), (n0, use_mask, use_label, got, want)
        if not use_mask and not use_label:
            assert (np.abs(got[np.isfinite(got)]) <= 1e-12).all()
        # survival: not increasing away from the anchor
        assert (np.diff(got[6:12 - n0]) <= 1e-12).all() and (np.diff(got[6 - n0:7]) >= -1e-12).all()
    print('anchor %d: worst |P twin - P enumerated| %.3e' % (n0, worst))


@pytest.mark.parametrize('n0', [0, 2, 5])
def test_right_walk_against_enumeration(n0):
    """The recursion of the device's right walk, restated over dense fa / W / post: U_n(s) = P(E on [n0, n] | c_n = s)."""
    f, T, mask, label, constrain = _small_chain()
    fa, W, post = extent_twin.dense_posterior(f, T)
    for use_mask, use_label in _EVENTS:
        mk, lb = (mask if use_mask else None), (label if use_label else None)
        got = extent_twin.right_walk(fa, W, post, n0, 6, mk, lb, constrain)
        want = _enumerated(f, T, n0, 0, 5 - n0, mk, lb, constrain)
        assert got.shape == want.shape == (6 - n0,)
        assert (np.abs(np.exp(got) - np.exp(want)) <= 1e-12).all(), (n0, use_mask, use_label, got, want)
    # the forward rows may carry any scale per segment, as the device's do
    scaled = fa * np.exp(np.random.RandomState(0).normal(scale=5., size=(6, 1)))
    assert np.abs(np.exp(extent_twin.right_walk(scaled, W, post, n0, 6, mask, label, constrain)) -
                  np.exp(extent_twin.right_walk(fa, W, post, n0, 6, mask, label, constrain))).max() <= 1e-12


class TwinBatch(object):
    """What posteriors.batch_event_extents needs of a RemixtBatch, answered by the twin: one dense (framelogprob,
    log_transmat) per restart."""

    def __init__(self, cn_classes, seg_class, framelogprobs, log_transmats, chain_start, chain_end):
        self.cn_classes = np.asarray(cn_classes)
        self.seg_class = np.asarray(seg_class)
        self.num_segments, self.num_cn_states = np.asarray(framelogprobs[0]).shape
        self.twins = [region_twin.RegionTwin(f, T, chain_start, chain_end) for f, T in zip(framelogprobs, log_transmats)]
        self.calls = []      # (nr, nq, wl, wr) of every call

    def region_extent_raw(self, r0, nr, queries, masks=None, labels=None, constrain=None, wl=0, wr=0):
        queries = np.asarray(queries).reshape(-1, 4)
        self.calls.append((nr, len(queries), wl, wr))
        out = np.zeros((nr, len(queries), wl + wr + 1))
        for i in range(nr):
            for j, (n0, mi, li, zero) in enumerate(queries):
                assert zero == 0
                mk = None if mi < 0 else np.asarray(masks)[self.seg_class, mi].astype(bool)
                lb = None if li < 0 else np.asarray(labels)[self.seg_class, li]
                out[i, j] = extent_twin.extent(self.twins[r0 + i], int(n0), wl, wr, mk, lb, constrain)
        return out


def _twin_batch(nr=2, seed=3):
    """Seven experiment segments in two chains; the model inserts zero-length segments at 2 and 6 (nine model segments)."""
    rng = np.random.RandomState(seed)
    S, M = 6, 2
    cn_classes = np.zeros((1, S, M, 2), dtype=int)
    cn_classes[0, :, 0] = (1, 1)
    cn_classes[0, :, 1] = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2)]
    N1 = 9
    tel = np.array([0, 0, 0, 0, 1, 0, 0, 0, 0])
    fs = [rng.normal(scale=1.5, size=(N1, S)) for _ in range(nr)]
    Ts = []
    for _ in range(nr):
        T = rng.normal(scale=1.5, size=(N1 - 1, S, S))
        T[4] = 0.
        Ts.append(T)
    cs, ce = posteriors.chains_from_telomeres(tel)
    b = TwinBatch(cn_classes, np.zeros(N1, dtype=int), fs, Ts, cs, ce)
    fwd = np.array([0, 1, 3, 4, 5, 7, 8])
    orig = np.ones(N1, dtype=bool); orig[[2, 6]] = False
    return b, fwd, orig, tel


def test_parse_event_and_window():
    assert posteriors.parse_event('loh') == (0, -1) and posteriors.parse_event('not_subclonal') == (5, -1)
    assert posteriors.parse_event('state') == (-1, 0) and posteriors.parse_event('total') == (-1, 1)
    assert posteriors.parse_event(('not_loh', 'total')) == (1, 1) and posteriors.parse_event((None, None)) == (-1, -1)
    assert posteriors.parse_event(['hdel', None]) == (2, -1)
    for ev in ((1, 1), (-1, -1), (5, 2)):
        assert posteriors.parse_event(posteriors.event_pair(ev)) == ev
    for bad in ('nothing', ('loh', 'nothing'), ('state', 'loh'), 3, ('loh',)):
        with pytest.raises(ValueError):
            posteriors.parse_event(bad)
    assert posteriors.parse_window(5) == (5, 5) and posteriors.parse_window((0, 7)) == (0, 7) and posteriors.parse_window(0) == (0, 0)
    assert posteriors.parse_window((2047, 2048)) == (2047, 2048)
    for bad in (-1, (3, -1), (2048, 2048), 2048):
        with pytest.raises(ValueError):
            posteriors.parse_window(bad)


def test_extent_queries():
    b, fwd, orig, tel = _twin_batch()
    q, constrain = posteriors.extent_queries([0, 2, 6], ('loh', 'state'), fwd, orig)
    assert q.dtype == np.int32 and q.tolist() == [[0, 0, 0, 0], [3, 0, 0, 0], [8, 0, 0, 0]]
    assert constrain.dtype == np.uint8 and constrain.tolist() == orig.astype(int).tolist()
    assert posteriors.extent_queries([4], 'total', fwd, orig)[0].tolist() == [[5, -1, 1, 0]]
    assert posteriors.extent_queries([], 'total', fwd, orig)[0].shape == (0, 4)
    for bad in ([7], [-1]):
        with pytest.raises(ValueError):
            posteriors.extent_queries(bad, 'total', fwd, orig)


def test_extent_summary_hand_made_curve():
    """One chain of 12 segments, no inserted ones; anchor 5, window (4, 5).  The right curve falls 1, .98, .6, .45, .04, .01
    and the chain goes on past the window; the left curve falls 1, .9, .3, .3, .02 and also stops inside the chain."""
    tel = np.zeros(12, dtype=int); tel[-1] = 1
    fwd = np.arange(12)
    p0 = 0.8
    right = np.array([1, .98, .6, .45, .04, .01])
    left = np.array([1, .9, .3, .3, .02])
    logp = np.log(p0 * np.concatenate([left[:0:-1], right]))
    s = posteriors.extent_summary(logp, 5, 4, 5, fwd, tel)
    assert abs(s['p_event'] - p0) <= 1e-14
    assert s['right_segments'].tolist() == [5, 6, 7, 8, 9, 10] and s['left_segments'].tolist() == [5, 4, 3, 2, 1]
    assert np.abs(s['right_survival'] - right).max() <= 1e-14 and np.abs(s['left_survival'] - left).max() <= 1e-14
    # the boundary pmf: the last segment the event reaches; the window's last entry is the censored mass
    assert np.abs(s['right_pmf'] - p0 * np.array([.02, .38, .15, .41, .03])).max() <= 1e-14 and abs(s['right_censored_mass'] - p0 * .01) <= 1e-14
    assert np.abs(s['left_pmf'] - p0 * np.array([.1, .6, 0., .28])).max() <= 1e-14 and abs(s['left_censored_mass'] - p0 * .02) <= 1e-14
    for side in ('right', 'left'):
        assert abs(s[side + '_pmf'].sum() + s[side + '_censored_mass'] - s['p_event']) <= 1e-14
    # right end R: P(R <= 5) = .02, P(R <= 6) = .4, P(R <= 7) = .55, P(R <= 8) = .96
    assert s['right_quantiles'].tolist() == [6, 7, 8] and s['right_censored'].tolist() == [False, False, False]
    # left end L: P(L <= 1) = .02 (censored), P(L <= 2) = P(L <= 3) = .3, P(L <= 4) = .9, P(L <= 5) = 1
    assert s['left_quantiles'].tolist() == [2, 4, 5] and s['left_censored'].tolist() == [False, False, False]
    # a curve that stays high: the quantiles fall in the censored mass and are reported as the window's end
    flat = np.log(p0 * np.concatenate([[.9, .98, .99, 1.], [1, .99, .98, .97, .965, .96]]))
    s = posteriors.extent_summary(flat, 5, 4, 5, fwd, tel)
    assert s['right_quantiles'].tolist() == [10, 10, 10] and s['right_censored'].tolist() == [True, True, True]
    assert s['left_quantiles'].tolist() == [1, 1, 2] and s['left_censored'].tolist() == [True, True, False]
    assert abs(s['right_censored_mass'] - p0 * .96) <= 1e-14 and abs(s['left_censored_mass'] - p0 * .9) <= 1e-14
    # the same curve in a chain that ends with the window: nothing is censored, the last segment takes the mass
    tel2 = tel.copy(); tel2[10] = 1; tel2[0] = 1
    s = posteriors.extent_summary(flat, 5, 4, 5, fwd, tel2)
    assert s['right_quantiles'].tolist() == [10, 10, 10] and not s['right_censored'].any() and s['right_censored_mass'] == 0
    assert s['left_quantiles'].tolist() == [1, 1, 2] and not s['left_censored'].any() and s['left_censored_mass'] == 0
    assert abs(s['right_pmf'][-1] - p0 * .96) <= 1e-14 and abs(s['left_pmf'][-1] - p0 * .9) <= 1e-14
    assert len(s['right_pmf']) == 6 and len(s['left_pmf']) == 5
    # an impossible event at the anchor
    s = posteriors.extent_summary(np.full(10, -np.inf), 5, 4, 5, fwd, tel)
    assert s['p_event'] == 0 and s['right_quantiles'].tolist() == [-1, -1, -1] and np.isnan(s['right_survival']).all()
    assert s['right_pmf'].sum() == 0 and s['left_pmf'].sum() == 0 and not s['left_censored'].any()
    with pytest.raises(ValueError):
        posteriors.extent_summary(np.zeros(9), 5, 4, 5, fwd, tel)
    c = posteriors.compact_extents([posteriors.extent_summary(flat, 5, 4, 5, fwd, tel), posteriors.extent_summary(logp, 5, 4, 5, fwd, tel)])
    assert sorted(c) == sorted(posteriors.EXTENT_ARRAYS)
    assert c['right_q50'].tolist() == [10, 7] and c['left_q05'].tolist() == [1, 2] and c['right_censored'].tolist() == [True, False]
    assert c['left_censored'].tolist() == [True, False] and np.abs(c['p_event'] - p0).max() <= 1e-14


def test_batch_event_extents():
    b, fwd, orig, tel = _twin_batch()
    masks, labels = posteriors.event_tables(b.cn_classes)
    anchors = [0, 2, 3, 4, 6]                      # model segments 0, 3, 4 (a chain end), 5 (a chain start), 8
    W = 3
    for event in ('not_loh', 'total', ('not_hdel', 'unphased'), (None, None)):
        mi, li = posteriors.parse_event(event)
        ncalls = len(b.calls)
        out = posteriors.batch_event_extents(b, 0, 2, anchors, event, W, fwd, orig, tel)
        assert b.calls[ncalls:] == [(2, len(anchors), W, W)]        # one device call per batch and event
        assert len(out) == 2 and all(len(o) == len(anchors) for o in out)
        mk = None if mi < 0 else masks[b.seg_class, mi].astype(bool)
        lb = None if li < 0 else labels[b.seg_class, li]
        for r in range(2):
            for j, a in enumerate(anchors):
                s = out[r][j]
                n0 = int(fwd[a])
                c0, c1 = (0, 4) if n0 <= 4 else (5, 8)
                # inserted segments (2 and 6) are dropped from the report; a window that crosses a chain end stops there
                want_r = [n for n in range(n0, min(n0 + W, c1) + 1) if orig[n]]
                want_l = [n for n in range(n0, max(n0 - W, c0) - 1, -1) if orig[n]]
                rev = dict((int(n), i) for i, n in enumerate(fwd))
                assert s['right_segments'].tolist() == [rev[n] for n in want_r] and s['left_segments'].tolist() == [rev[n] for n in want_l]
                p0 = np.exp(b.twins[r].logprob(n0, n0, mk, lb, orig))
                assert abs(s['p_event'] - p0) <= 1e-12
                for side, segs in (('right', want_r), ('left', want_l)):
                    surv = s[side + '_survival']
                    want = np.array([np.exp(b.twins[r].logprob(min(n, n0), max(n, n0), mk, lb, orig)) for n in segs]) / p0
                    assert np.abs(surv - want).max() <= 1e-12, (event, r, a, side)
                    assert surv[0] == 1 and (np.diff(surv) <= 0).all()                      # monotone curves
                    assert abs(s[side + '_pmf'].sum() + s[side + '_censored_mass'] - s['p_event']) <= 1e-12
                    q = s[side + '_quantiles']
                    assert (np.diff(q) >= 0).all() and np.isin(q, s[side + '_segments']).all()
                    more = (segs[-1] + 1 <= c1 and orig[segs[-1] + 1:c1 + 1].any()) if side == 'right' else (segs[-1] - 1 >= c0 and orig[c0:segs[-1]].any())
                    assert (s[side + '_censored_mass'] > 0) == bool(more)
                    assert len(s[side + '_pmf']) == len(segs) - (1 if more else 0)
                    if not more:
                        assert not s[side + '_censored'].any()
                assert (s['left_quantiles'] <= a).all() and (s['right_quantiles'] >= a).all()
                if event == (None, None):
                    assert abs(s['p_event'] - 1) <= 1e-12 and np.abs(s['right_survival'] - 1).max() <= 1e-12
        # a chain end: the anchor at segment 3 (model 4) has nothing to its right, the one at 4 (model 5) nothing to its left
        assert out[0][2]['right_segments'].tolist() == [3] and out[0][3]['left_segments'].tolist() == [4]
        assert out[0][2]['right_quantiles'].tolist() == [3, 3, 3] and abs(out[0][2]['right_pmf'][0] - out[0][2]['p_event']) <= 1e-15
    # restart range, an uneven window, and no anchors: no device call
    one = posteriors.batch_event_extents(b, 1, 1, anchors, 'total', W, fwd, orig, tel)
    both = posteriors.batch_event_extents(b, 0, 2, anchors, 'total', W, fwd, orig, tel)
    assert all(np.array_equal(one[0][j][k], both[1][j][k]) for j in range(len(anchors)) for k in one[0][j])
    wide = posteriors.batch_event_extents(b, 0, 1, [2], 'total', (1, 4), fwd, orig, tel)[0][0]
    assert b.calls[-1] == (1, 1, 1, 4) and wide['left_segments'].tolist() == [2] and wide['right_segments'].tolist() == [2, 3]
    ncalls = len(b.calls)
    assert posteriors.batch_event_extents(b, 0, 2, [], 'total', W, fwd, orig, tel) == [[], []] and len(b.calls) == ncalls
    # entries of several events, grouped: one call per distinct event, the arrays in entry order
    names, anc, events = posteriors.parse_extents([('a', 0, 'total'), ('b', 4, 'not_loh'), ('c', 6, 'total')])
    assert names == ['a', 'b', 'c'] and anc.tolist() == [0, 4, 6] and events == [(-1, 1), (1, -1), (-1, 1)]
    ncalls = len(b.calls)
    fn = lambda a, ev, w: posteriors.batch_event_extents(b, 0, 2, a, ev, w, fwd, orig, tel)
    got = posteriors.grouped_event_extents(fn, anc, events, (W, W))
    assert sorted(c[:2] for c in b.calls[ncalls:]) == [(2, 1), (2, 2)] and len(got) == 2
    for r in range(2):
        assert sorted(got[r]) == sorted(posteriors.EXTENT_ARRAYS)
        tot = posteriors.compact_extents(posteriors.batch_event_extents(b, r, 1, [0, 6], 'total', W, fwd, orig, tel)[0])
        loh = posteriors.compact_extents(posteriors.batch_event_extents(b, r, 1, [4], 'not_loh', W, fwd, orig, tel)[0])
        for k in posteriors.EXTENT_ARRAYS:
            assert got[r][k].shape == (3,) and got[r][k][[0, 2]].tolist() == tot[k].tolist() and got[r][k][1] == loh[k][0], k
        assert got[r]['left_q05'].dtype == np.int64 and got[r]['right_censored'].dtype == bool and got[r]['p_event'].dtype == float


def _fake_extents(rng, A):
    out = {'p_event': rng.uniform(size=A)}
    for k in posteriors.EXTENT_ARRAYS[1:7]:
        out[k] = rng.randint(0, 40, size=A)
    for k in posteriors.EXTENT_ARRAYS[7:]:
        out[k] = rng.uniform(size=A) < 0.5
    return out


def test_record_round_trip_and_unchanged_when_off():
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=4, num_chains=3, seed=2)
    ps = synthetic.make_init_params(e, 3, 4)
    rng = np.random.RandomState(0)
    names = ['negbin_r_0', 'negbin_r_1', 'betabin_M_0', 'betabin_M_1']
    N, M = len(e.x), 3
    brk_ids = list(e.breakpoints.keys())
    region_names = ['geneA', 'arm']
    extent_names = ['del', 'run', 'loh']
    A = len(extent_names)
    full = []
    for _ in ps:
        r2 = _fake_result(e, rng)
        posteriors.add_region_events(r2, region_names, dict((k, rng.uniform(size=2)) for k in posteriors.REGION_ARRAYS))
        posteriors.add_event_extents(r2, extent_names, _fake_extents(rng, A))
        got = r2['event_extents']
        assert sorted(got) == sorted(('names',) + posteriors.EXTENT_ARRAYS) and all(len(got[k]) == A for k in posteriors.EXTENT_ARRAYS)
        full.append(r2)
    nb = len(brk_ids)
    for b in full:
        for kw in (dict(), dict(region_names=region_names)):
            # off: the vectors of a call that omits the keyword
            f0, i0 = restarts._pack(b, N, M, nb, 4, brk_ids, names, **kw)
            f1, i1 = restarts._pack(b, N, M, nb, 4, brk_ids, names, extent_names=None, **kw)
            assert f0.tobytes() == f1.tobytes() and i0.tobytes() == i1.tobytes()
            # on: the section after everything else, nine floats per entry
            f2, i2 = restarts._pack(b, N, M, nb, 4, brk_ids, names, extent_names=extent_names, **kw)
            assert len(f2) == len(f0) + 9 * A and f2[:len(f0)].tobytes() == f0.tobytes() and i2.tobytes() == i0.tobytes()
            assert np.array_equal(f2[len(f0):len(f0) + A], b['event_extents']['p_event'])
            assert np.array_equal(f2[-A:], b['event_extents']['right_censored'].astype(float))
    off = restarts.gather_result_records(full, e, ps, M, names, region_names=region_names)
    on = restarts.gather_result_records(full, e, ps, M, names, region_names=region_names, extent_names=extent_names)
    only = restarts.gather_result_records(full, e, ps, M, names, extent_names=extent_names)
    for i, res in on.items():
        assert 'event_extents' not in off[i] and sorted(set(res) - {'event_extents'}) == sorted(off[i])
        assert sorted(res['stats']) == sorted(off[i]['stats'])
        for got in (res, only[i]):
            assert got['event_extents']['names'] == extent_names
            for k in posteriors.EXTENT_ARRAYS:
                assert got['event_extents'][k].dtype == full[i]['event_extents'][k].dtype, k
                assert np.array_equal(got['event_extents'][k], full[i]['event_extents'][k]), k
        assert 'region_events' not in only[i]
        for k in posteriors.REGION_ARRAYS:
            assert np.array_equal(res['region_events'][k], full[i]['region_events'][k]), k


def test_config():
    assert defaults.cn_event_extents is None and defaults.get_param({}, 'cn_event_extents') is None
    assert defaults.cn_extent_window == 64 and defaults.get_param({}, 'cn_extent_window') == 64
    assert posteriors.extents_on({}) is None and posteriors.extents_on({'cn_extent_window': 5}) is None
    names, anchors, events, window = posteriors.extents_on({'cn_event_extents': [('del', 3, 'loh'), ('run', 7, ('not_loh', 'total'))]})
    assert names == ['del', 'run'] and anchors.tolist() == [3, 7] and events == [(0, -1), (1, 1)] and window == (64, 64)
    assert posteriors.extents_on({'cn_event_extents': [], 'cn_extent_window': (2, 9)})[3] == (2, 9)
    bad = [[('a', 3)], [('a', -1, 'loh')], [('a', 3, 'nothing')], [('a', 2.5, 'loh')], ['abc']]
    for ext in bad:
        with pytest.raises(ValueError):
            posteriors.extents_on({'cn_event_extents': ext})
    with pytest.raises(ValueError):
        posteriors.extents_on({'cn_event_extents': [('a', 3, 'loh')], 'cn_extent_window': 4096})
    with pytest.raises(ValueError, match='outside the experiment'):
        posteriors.extents_on({'cn_event_extents': [('a', 20, 'loh')]}, num_segments=20)
    # the entry points refuse a bad entry before any fit
    from remixt_amd.analysis import pipeline
    e = synthetic.make_experiment(20, num_clones=3, max_copy_number=3, num_chains=2, seed=0)
    ps = synthetic.make_init_params(e, 2, 3)
    for ext, text in (([('a', 20, 'loh')], 'outside the experiment'), ([('a', 3, 'nothing')], 'unknown event')):
        with pytest.raises(ValueError, match=text):
            pipeline.fit_restarts(e, dict(enumerate(ps)), {'cn_event_extents': ext})
        with pytest.raises(ValueError, match=text):
            pipeline.fit(e, ps[0], {'cn_event_extents': ext})
        with pytest.raises(ValueError, match=text):
            restarts.fit_restarts_distributed(e, ps, 3, cn_event_extents=ext)


def test_oracle_module_has_no_event_extent():
    from oracle import oracle
    from tests import helpers as H
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError):
        mo.event_extent([3], 'loh')


def test_declared_and_bound():
    import os
    from remixt_amd import _lib
    assert 'rmx_region_extent' in _lib.SYMBOLS and len(_lib.SYMBOLS['rmx_region_extent'][1]) == 13
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'remixt_amd.h')) as fh:
        text = fh.read()
    assert 'int rmx_region_extent(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries' in text
    assert 'int32_t wl, int32_t wr, double *logp_out);' in text
    with open(os.path.join(root, 'remixt_amd', 'csrc', 'rmx_api.hip')) as fh:
        api = fh.read()
    assert '"k_region_moments", "k_region_extent"};' in api and 'KID_REGION_MOMENTS, KID_REGION_EXTENT, KID_COUNT' in api
