"""Host side of the region event spans (remixt_amd/posteriors.py) and their numpy twin, without a GPU: the twin and the
restated column recursion against brute-force path enumeration, span_summary / batch_event_spans against a batch answered
by the twin and against extent_summary, quantiles and length_cdf on a hand-made table, grouped_event_spans, the distributed
record with and without the section, the config checks, the declarations."""
import numpy as np
import pytest

from remixt_amd import posteriors
from tests import extent_twin, region_twin, span_twin
from tests.test_region_extent_cpu import _EVENTS, TwinBatch, _small_chain, _twin_batch


def _enumerated(f, T, n0, wl, wr, mask, label, constrain):
    N = len(f)
    out = np.full((wl + 1, wr + 1), -np.inf)
    for a in range(wl + 1):
        for c in range(wr + 1):
            if n0 - a >= 0 and n0 + c < N:
                out[a, c] = region_twin.brute_force(f, T, n0 - a, n0 + c, mask, label, constrain)
    return out


@pytest.fixture(scope='module')
def enumerated():
    """The enumerated tables of the small chain, window (6, 6): {(n0, use_mask, use_label): table}, computed once."""
    f, T, mask, label, constrain = _small_chain()
    return dict(((n0, um, ul), _enumerated(f, T, n0, 6, 6, mask if um else None, label if ul else None, constrain))
                for n0 in (0, 2, 5) for um, ul in _EVENTS)


@pytest.mark.parametrize('n0', [0, 2, 5])
def test_twin_against_enumeration(n0, enumerated):
    f, T, mask, label, constrain = _small_chain()
    twin = region_twin.RegionTwin(f, T, [0], [5])
    worst = 0.
    for use_mask, use_label in _EVENTS:
        mk, lb = (mask if use_mask else None), (label if use_label else None)
        got = span_twin.span(twin, n0, 6, 6, mk, lb, constrain)
        want = enumerated[n0, use_mask, use_label]
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        # outside the chain: -inf; inside: finite
        assert np.isneginf(got[n0 + 1:]).all() and np.isneginf(got[:, 6 - n0:]).all() and np.isfinite(got[:n0 + 1, :6 - n0]).all()
        err = np.abs(np.exp(got) - np.exp(want))
        worst = max(worst, err.max())
        assert (err <= 1e-12).all(), (n0, use_mask, use_label, got, want)
        if not use_mask and not use_label:
            assert (np.abs(got[np.isfinite(got)]) <= 1e-12).all()
        # the table does not increase in a or in c
        inside = got[:n0 + 1, :6 - n0]
        assert (np.diff(inside, axis=0) <= 1e-12).all() and (np.diff(inside, axis=1) <= 1e-12).all()
        # row 0 and column 0 are the two halves of the extent twin's row
        row = extent_twin.extent(twin, n0, 6, 6, mk, lb, constrain)
        assert np.array_equal(got[0], row[6:]) and np.array_equal(got[:, 0], row[6::-1])
    print('anchor %d: worst |P twin - P enumerated| %.3e' % (n0, worst))


@pytest.mark.parametrize('n0', [0, 2, 5])
def test_column_walk_against_enumeration(n0, enumerated):
    """The device's recursion restated over dense fa / W / post: one column per right end, each scaled on its own."""
    f, T, mask, label, constrain = _small_chain()
    fa, W, post = extent_twin.dense_posterior(f, T)
    for use_mask, use_label in _EVENTS:
        mk, lb = (mask if use_mask else None), (label if use_label else None)
        got = span_twin.column_walk(fa, W, post, n0, 6, 6, mk, lb, constrain)
        want = enumerated[n0, use_mask, use_label]
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        assert (np.abs(np.exp(got) - np.exp(want)) <= 1e-12).all(), (n0, use_mask, use_label, got, want)
        # a narrower window gives the entries it shares
        part = span_twin.column_walk(fa, W, post, n0, 1, 2, mk, lb, constrain)
        assert np.array_equal(part, got[:2, :3])
    # the forward rows may carry any scale per segment, as the device's do
    scaled = fa * np.exp(np.random.RandomState(0).normal(scale=5., size=(6, 1)))
    assert np.abs(np.exp(span_twin.column_walk(scaled, W, post, n0, 6, 6, mask, label, constrain)) -
                  np.exp(span_twin.column_walk(fa, W, post, n0, 6, 6, mask, label, constrain))).max() <= 1e-12


class SpanTwinBatch(TwinBatch):
    """TwinBatch with region_span_raw answered by the twin."""

    def region_span_raw(self, r0, nr, queries, masks=None, labels=None, constrain=None, wl=0, wr=0):
        queries = np.asarray(queries).reshape(-1, 4)
        self.calls.append(('span', nr, len(queries), wl, wr))
        out = np.zeros((nr, len(queries), wl + 1, wr + 1))
        for i in range(nr):
            for j, (n0, mi, li, zero) in enumerate(queries):
                assert zero == 0
                mk = None if mi < 0 else np.asarray(masks)[self.seg_class, mi].astype(bool)
                lb = None if li < 0 else np.asarray(labels)[self.seg_class, li]
                out[i, j] = span_twin.span(self.twins[r0 + i], int(n0), wl, wr, mk, lb, constrain)
        return out


def _span_batch():
    b, fwd, orig, tel = _twin_batch()
    b.__class__ = SpanTwinBatch
    l1 = np.array([3., 5., 0., 7., 11., 13., 0., 17., 19.])      # (the inserted segments 2 and 6 have no length)
    return b, fwd, orig, tel, l1


def test_parse_span_window():
    assert posteriors.parse_span_window(5) == (5, 5) and posteriors.parse_span_window((0, 7)) == (0, 7)
    assert posteriors.parse_span_window(127) == (127, 127) and posteriors.parse_span_window((0, 16383)) == (0, 16383)
    for bad in (-1, (3, -1), 128, (127, 128), (1, 8192)):
        with pytest.raises(ValueError):
            posteriors.parse_span_window(bad)


def _hand_made():
    """One chain of 12 segments, no inserted ones; anchor 5, window (2, 3); segment n is 10 (n + 1) long.  The joint pmf of
    (left end, right end) given the event, rows L = 5, 4, 3 and columns R = 5, 6, 7, 8."""
    pmf = np.array([[.10, .05, .05, .00], [.05, .20, .10, .05], [.00, .10, .20, .10]])
    J = pmf[::-1, ::-1].cumsum(axis=0).cumsum(axis=1)[::-1, ::-1]
    p0 = 0.8
    return pmf, np.log(p0 * J), p0, 10. * (np.arange(12) + 1)


def test_span_summary_hand_made_table():
    pmf, logp, p0, l1 = _hand_made()
    fwd = np.arange(12)
    tel = np.zeros(12, dtype=int); tel[-1] = 1
    lengths = np.array([[60, 130, 210, 300], [110, 180, 260, 350], [150, 220, 300, 390]], dtype=float)
    # open on both sides: the last row and the last column are lumps "at or beyond"
    s = posteriors.span_summary(logp, 5, 2, 3, fwd, tel, l1)
    assert abs(s['p_event'] - p0) <= 1e-14 and s['left_open'] and s['right_open']
    assert s['left_segments'].tolist() == [5, 4, 3] and s['right_segments'].tolist() == [5, 6, 7, 8]
    assert np.abs(s['joint_pmf'] - p0 * pmf).max() <= 1e-14 and abs(s['joint_pmf'].sum() - p0) <= 1e-14
    assert s['joint_survival'][0, 0] == 1 and abs(s['joint_survival'][1, 2] - .45) <= 1e-14      # (.10 + .05 + .20 + .10)
    assert np.array_equal(s['lengths'], lengths)
    # closed cells in increasing length: 60 (.10), 110 (.15), 130 (.20), 180 (.40), 210 (.45), 260 (.55): the closed mass ends at .55
    assert s['length_quantiles'].tolist() == [60., 260., 390.] and s['length_censored'].tolist() == [False, False, True]
    p_le, p_un = s['length_cdf']([100, 200, 400])
    assert np.abs(p_le - [.10, .40, .55]).max() <= 1e-14 and np.abs(p_un - [0, 0, .45]).max() <= 1e-14
    p_le, p_un = s['length_cdf']([320])
    assert abs(p_le[0] - .55) <= 1e-14 and abs(p_un[0] - .30) <= 1e-14      # open cells with a lower bound <= 320: 150, 220, 300, 300
    # open on the right only: the chain starts at segment 3
    tel1 = tel.copy(); tel1[2] = 1
    s = posteriors.span_summary(logp, 5, 2, 3, fwd, tel1, l1)
    assert not s['left_open'] and s['right_open'] and np.abs(s['joint_pmf'] - p0 * pmf).max() <= 1e-14
    assert s['length_quantiles'].tolist() == [60., 220., 390.] and s['length_censored'].tolist() == [False, False, True]
    p_le, p_un = s['length_cdf']([100, 200, 400])
    assert np.abs(p_le - [.10, .40, .85]).max() <= 1e-14 and np.abs(p_un - [0, 0, .15]).max() <= 1e-14
    # closed on both sides: the chain is the window
    tel2 = tel1.copy(); tel2[8] = 1
    s = posteriors.span_summary(logp, 5, 2, 3, fwd, tel2, l1)
    assert not s['left_open'] and not s['right_open']
    assert s['length_quantiles'].tolist() == [60., 220., 390.] and not s['length_censored'].any()
    p_le, p_un = s['length_cdf']([100, 200, 400])
    assert np.abs(p_le - [.10, .40, 1.]).max() <= 1e-14 and (p_un == 0).all()
    # rounding that makes the table rise is removed by the running minimum along both axes, and what is left of it is clipped
    bumped = logp.copy(); bumped[1, 2] += 1e-13; bumped[2, 1] += 1e-13
    s = posteriors.span_summary(bumped, 5, 2, 3, fwd, tel, l1)
    assert (s['joint_pmf'] >= 0).all() and abs(s['joint_pmf'].sum() - p0) <= 1e-12
    assert (np.diff(s['joint_survival'], axis=0) <= 0).all() and (np.diff(s['joint_survival'], axis=1) <= 0).all()
    # an impossible event at the anchor
    s = posteriors.span_summary(np.full((3, 4), -np.inf), 5, 2, 3, fwd, tel, l1)
    assert s['p_event'] == 0 and s['length_quantiles'].tolist() == [-1, -1, -1] and not s['length_censored'].any()
    assert np.isnan(s['joint_survival']).all() and s['joint_pmf'].sum() == 0 and np.isnan(s['length_cdf']([100])[0]).all()
    with pytest.raises(ValueError):
        posteriors.span_summary(np.zeros((4, 3)), 5, 2, 3, fwd, tel, l1)
    # compact_spans: the arrays of a fit result
    both = [posteriors.span_summary(logp, 5, 2, 3, fwd, t, l1) for t in (tel, tel2)]
    c = posteriors.compact_spans(both, edges=[100, 400])
    assert sorted(c) == sorted(posteriors.SPAN_ARRAYS + posteriors.SPAN_EDGE_ARRAYS)
    assert c['length_q50'].tolist() == [260., 220.] and c['length_q95'].tolist() == [390., 390.] and c['length_censored'].tolist() == [True, False]
    assert c['p_length_le'].shape == (2, 2) and np.abs(c['p_length_le'] - [[.10, .55], [.10, 1.]]).max() <= 1e-14
    assert np.abs(c['p_length_undetermined'] - [[0, .45], [0, 0]]).max() <= 1e-14
    assert posteriors.compact_spans(both)['p_length_le'].shape == (2, 0)


def test_batch_event_spans():
    b, fwd, orig, tel, l1 = _span_batch()
    masks, labels = posteriors.event_tables(b.cn_classes)
    anchors = [0, 2, 3, 4, 6]                      # model segments 0, 3, 4 (a chain end), 5 (a chain start), 8
    W = 3
    rev = dict((int(n), i) for i, n in enumerate(fwd))
    for event in ('not_loh', 'total', ('not_hdel', 'unphased'), (None, None)):
        mi, li = posteriors.parse_event(event)
        ncalls = len(b.calls)
        out = posteriors.batch_event_spans(b, 0, 2, anchors, event, W, fwd, orig, tel, l1)
        assert b.calls[ncalls:] == [('span', 2, len(anchors), W, W)]        # one device call per batch and event
        ext = posteriors.batch_event_extents(b, 0, 2, anchors, event, W, fwd, orig, tel)
        mk = None if mi < 0 else masks[b.seg_class, mi].astype(bool)
        lb = None if li < 0 else labels[b.seg_class, li]
        for r in range(2):
            for j, a in enumerate(anchors):
                s, x = out[r][j], ext[r][j]
                n0 = int(fwd[a])
                c0, c1 = (0, 4) if n0 <= 4 else (5, 8)
                # inserted segments (2 and 6) are dropped; a window that crosses a chain end stops there
                want_r = [n for n in range(n0, min(n0 + W, c1) + 1) if orig[n]]
                want_l = [n for n in range(n0, max(n0 - W, c0) - 1, -1) if orig[n]]
                assert s['right_segments'].tolist() == [rev[n] for n in want_r] == x['right_segments'].tolist()
                assert s['left_segments'].tolist() == [rev[n] for n in want_l] == x['left_segments'].tolist()
                assert s['right_open'] == (x['right_censored_mass'] > 0) and s['left_open'] == (x['left_censored_mass'] > 0)
                assert abs(s['p_event'] - x['p_event']) <= 1e-15
                want = np.array([[np.exp(b.twins[r].logprob(nl, nr, mk, lb, orig)) for nr in want_r] for nl in want_l]) / s['p_event']
                assert np.abs(s['joint_survival'] - want).max() <= 1e-12, (event, r, a)
                pmf = s['joint_pmf']
                assert pmf.shape == (len(want_l), len(want_r)) == s['lengths'].shape
                assert (pmf >= 0).all() and abs(pmf.sum() - s['p_event']) <= 1e-12
                # the marginals of the joint pmf are extent_summary's boundary pmfs, followed by the censored mass where there is one
                for axis, side in ((1, 'left'), (0, 'right')):
                    marg = np.append(x[side + '_pmf'], x[side + '_censored_mass']) if s[side + '_open'] else x[side + '_pmf']
                    assert np.abs(pmf.sum(axis=axis) - marg).max() <= 1e-12, (event, r, a, side)
                assert np.array_equal(s['lengths'], np.array([[l1[nl:nr + 1].sum() for nr in want_r] for nl in want_l]))
                q = s['length_quantiles']
                assert (np.diff(q) >= 0).all() and np.isin(q, s['lengths']).all()
                closed = np.ones(pmf.shape, dtype=bool)
                closed[-1, :] &= not s['left_open']; closed[:, -1] &= not s['right_open']
                p_le, p_un = s['length_cdf']([0., 1e9])
                assert p_le[0] == 0 and p_un[0] == 0 and abs(p_le[1] + p_un[1] - 1) <= 1e-12
                assert abs(p_le[1] - pmf[closed].sum() / s['p_event']) <= 1e-12
                assert (s['length_censored'] == (p_le[1] < np.array(posteriors.EXTENT_QUANTILES))).all()
                if event == (None, None):
                    assert abs(s['p_event'] - 1) <= 1e-12 and np.abs(s['joint_survival'] - 1).max() <= 1e-12
                    # everything sits in the farthest cell
                    assert abs(pmf[-1, -1] - 1) <= 1e-12
        # a chain end: the anchor at segment 3 (model 4) has nothing to its right, the one at 4 (model 5) nothing to its left
        assert out[0][2]['right_segments'].tolist() == [3] and not out[0][2]['right_open']
        assert out[0][3]['left_segments'].tolist() == [4] and not out[0][3]['left_open']
    # restart range, an uneven window, and no anchors: no device call
    one = posteriors.batch_event_spans(b, 1, 1, anchors, 'total', W, fwd, orig, tel, l1)
    both = posteriors.batch_event_spans(b, 0, 2, anchors, 'total', W, fwd, orig, tel, l1)
    assert all(np.array_equal(one[0][j][k], both[1][j][k], equal_nan=True) for j in range(len(anchors)) for k in one[0][j] if k != 'length_cdf')
    wide = posteriors.batch_event_spans(b, 0, 1, [2], 'total', (1, 4), fwd, orig, tel, l1)[0][0]
    assert b.calls[-1] == ('span', 1, 1, 1, 4) and wide['left_segments'].tolist() == [2] and wide['right_segments'].tolist() == [2, 3]
    assert wide['joint_pmf'].shape == (1, 2) and not wide['right_open'] and wide['left_open']
    ncalls = len(b.calls)
    assert posteriors.batch_event_spans(b, 0, 2, [], 'total', W, fwd, orig, tel, l1) == [[], []] and len(b.calls) == ncalls
    with pytest.raises(ValueError):
        posteriors.batch_event_spans(b, 0, 2, anchors, 'total', 128, fwd, orig, tel, l1)


def test_oracle_module_has_no_event_span():
    from oracle import oracle
    from tests import helpers as H
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError):
        mo.event_span([3], 'loh')


def test_declared_and_bound():
    import os
    from remixt_amd import _lib, bpmodel, restarts
    assert 'rmx_region_span' in _lib.SYMBOLS and len(_lib.SYMBOLS['rmx_region_span'][1]) == 13
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'remixt_amd.h')) as fh:
        text = fh.read()
    assert 'int rmx_region_span(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries' in text
    with open(os.path.join(root, 'remixt_amd', 'csrc', 'rmx_api.hip')) as fh:
        api = fh.read()
    # the profile id is appended after k_region_extent
    assert '"k_region_extent", "k_region_span"};' in api and 'KID_REGION_EXTENT, KID_REGION_SPAN, KID_COUNT\n' in api
    assert hasattr(bpmodel.RemixtBatch, 'region_span_raw') and hasattr(bpmodel.RemixtModel, 'region_span')
    for cls in (restarts.RestartSet, restarts.RestartGroups, restarts.DatasetGroups):
        assert hasattr(cls, 'event_span')


def test_grouped_event_spans():
    b, fwd, orig, tel, l1 = _span_batch()
    names, anc, events = posteriors.parse_extents([('a', 0, 'total'), ('b', 4, 'not_loh'), ('c', 6, 'total')])
    ncalls = len(b.calls)
    fn = lambda a, ev, w: posteriors.batch_event_spans(b, 0, 2, a, ev, w, fwd, orig, tel, l1)
    edges = (10., 40.)
    got = posteriors.grouped_event_spans(fn, anc, events, (3, 3), edges)
    assert sorted(c[1:3] for c in b.calls[ncalls:]) == [(2, 1), (2, 2)] and len(got) == 2      # one call per distinct event
    keys = posteriors.SPAN_ARRAYS + posteriors.SPAN_EDGE_ARRAYS
    for r in range(2):
        assert sorted(got[r]) == sorted(keys)
        tot = posteriors.compact_spans(posteriors.batch_event_spans(b, r, 1, [0, 6], 'total', 3, fwd, orig, tel, l1)[0], edges)
        loh = posteriors.compact_spans(posteriors.batch_event_spans(b, r, 1, [4], 'not_loh', 3, fwd, orig, tel, l1)[0], edges)
        for k in keys:
            assert got[r][k].shape == ((3,) if k in posteriors.SPAN_ARRAYS else (3, 2)), k
            assert np.array_equal(got[r][k][[0, 2]], tot[k]) and np.array_equal(got[r][k][1], loh[k][0]), k
        assert got[r]['length_censored'].dtype == bool and got[r]['length_q50'].dtype == float
        assert ((got[r]['p_length_le'] >= 0) & (got[r]['p_length_le'] + got[r]['p_length_undetermined'] <= 1 + 1e-12)).all()
    assert posteriors.grouped_event_spans(fn, anc, events, (3, 3))[0]['p_length_le'].shape == (3, 0)


def _fake_lengths(rng, A, E):
    out = dict((k, rng.uniform(1., 1e6, size=A)) for k in posteriors.SPAN_ARRAYS[:3])
    out['length_censored'] = rng.uniform(size=A) < 0.5
    for k in posteriors.SPAN_EDGE_ARRAYS:
        out[k] = rng.uniform(size=(A, E))
    return out


def test_record_round_trip_and_unchanged_when_off():
    from remixt_amd import restarts, synthetic
    from tests.test_cn_samples_records_cpu import _fake_result
    from tests.test_region_extent_cpu import _fake_extents
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=4, num_chains=3, seed=2)
    ps = synthetic.make_init_params(e, 3, 4)
    rng = np.random.RandomState(0)
    names = ['negbin_r_0', 'negbin_r_1', 'betabin_M_0', 'betabin_M_1']
    N, M = len(e.x), 3
    brk_ids = list(e.breakpoints.keys())
    extent_names = ['del', 'run', 'loh']
    A = len(extent_names)
    for E in (0, 2):
        full = []
        for _ in ps:
            r2 = _fake_result(e, rng)
            posteriors.add_event_extents(r2, extent_names, _fake_extents(rng, A))
            posteriors.add_event_lengths(r2, extent_names, _fake_lengths(rng, A, E))
            got = r2['event_lengths']
            assert sorted(got) == sorted(('names',) + posteriors.SPAN_ARRAYS + posteriors.SPAN_EDGE_ARRAYS)
            full.append(r2)
        nb = len(brk_ids)
        for b in full:
            # off: the vectors of a call that omits the keyword
            f0, i0 = restarts._pack(b, N, M, nb, 4, brk_ids, names, extent_names=extent_names)
            f1, i1 = restarts._pack(b, N, M, nb, 4, brk_ids, names, extent_names=extent_names, length_edges=None)
            assert f0.tobytes() == f1.tobytes() and i0.tobytes() == i1.tobytes()
            # on: the section at the end, after the extents, (4 + 2 edges) floats per entry
            f2, i2 = restarts._pack(b, N, M, nb, 4, brk_ids, names, extent_names=extent_names, length_edges=E)
            assert len(f2) == len(f0) + (4 + 2 * E) * A and f2[:len(f0)].tobytes() == f0.tobytes() and i2.tobytes() == i0.tobytes()
            assert np.array_equal(f2[len(f0):len(f0) + A], b['event_lengths']['length_q05'])
            assert np.array_equal(f2[len(f0) + 3 * A:len(f0) + 4 * A], b['event_lengths']['length_censored'].astype(float))
            assert np.array_equal(f2[len(f0) + 4 * A:], np.concatenate([b['event_lengths'][k].ravel() for k in posteriors.SPAN_EDGE_ARRAYS]))
        off = restarts.gather_result_records(full, e, ps, M, names, extent_names=extent_names)
        on = restarts.gather_result_records(full, e, ps, M, names, extent_names=extent_names, length_edges=E)
        for i, res in on.items():
            assert 'event_lengths' not in off[i] and sorted(set(res) - {'event_lengths'}) == sorted(off[i])
            assert res['event_lengths']['names'] == extent_names
            for k in posteriors.SPAN_ARRAYS + posteriors.SPAN_EDGE_ARRAYS:
                assert res['event_lengths'][k].dtype == full[i]['event_lengths'][k].dtype, k
                assert np.array_equal(res['event_lengths'][k], full[i]['event_lengths'][k]), k
            for k in posteriors.EXTENT_ARRAYS:
                assert np.array_equal(res['event_extents'][k], full[i]['event_extents'][k]), k


def test_config():
    from remixt_amd import defaults, restarts, synthetic
    assert defaults.cn_event_lengths is False and defaults.get_param({}, 'cn_event_lengths') is False
    assert defaults.cn_event_length_edges == () and defaults.get_param({}, 'cn_event_length_edges') == ()
    ext = [('del', 3, 'loh'), ('run', 7, ('not_loh', 'total'))]
    assert posteriors.lengths_on({}) is None and posteriors.lengths_on({'cn_event_extents': ext}) is None
    assert posteriors.lengths_on({'cn_event_extents': ext, 'cn_event_length_edges': [1e6]}) is None
    names, anchors, events, window, edges = posteriors.lengths_on({'cn_event_extents': ext, 'cn_event_lengths': True, 'cn_event_length_edges': [3e6, 1e7]})
    assert names == ['del', 'run'] and anchors.tolist() == [3, 7] and events == [(0, -1), (1, 1)] and window == (64, 64) and edges == (3e6, 1e7)
    assert posteriors.lengths_on({'cn_event_extents': ext, 'cn_event_lengths': True, 'cn_extent_window': 127})[3:] == ((127, 127), ())
    with pytest.raises(ValueError, match='needs cn_event_extents'):
        posteriors.lengths_on({'cn_event_lengths': True})
    with pytest.raises(ValueError, match='16384 entries'):
        posteriors.lengths_on({'cn_event_extents': ext, 'cn_event_lengths': True, 'cn_extent_window': 128})
    for bad in ([0.], [-1.], [1e6, np.nan], 5., ['x']):
        with pytest.raises(ValueError, match='cn_event_length_edges'):
            posteriors.lengths_on({'cn_event_extents': ext, 'cn_event_lengths': True, 'cn_event_length_edges': bad})
    # the entry points refuse a bad combination before any fit
    from remixt_amd.analysis import pipeline
    e = synthetic.make_experiment(20, num_clones=3, max_copy_number=3, num_chains=2, seed=0)
    ps = synthetic.make_init_params(e, 2, 3)
    for cfg, text in (({'cn_event_lengths': True}, 'needs cn_event_extents'),
                      ({'cn_event_lengths': True, 'cn_event_extents': ext, 'cn_extent_window': 128}, '16384 entries'),
                      ({'cn_event_lengths': True, 'cn_event_extents': ext, 'cn_event_length_edges': [0.]}, 'must be > 0')):
        with pytest.raises(ValueError, match=text):
            pipeline.fit_restarts(e, dict(enumerate(ps)), cfg)
        with pytest.raises(ValueError, match=text):
            pipeline.fit(e, ps[0], cfg)
        with pytest.raises(ValueError, match=text):
            restarts.fit_restarts_distributed(e, ps, 3, **cfg)
