"""Region event spans on the device (rmx_region_span / k_region_span): every entry against the numpy twin (RegionTwin.logprob
per interval) on the read-back framelogprob / log_transmat, against rmx_region_prob on the same interval and against
rmx_region_extent on row 0 and column 0; the exact identities, two state classes, the mixed-model state, degenerate
windows, bit identity across restart ranges, query batches, windows and restart groups, no side effects on the model,
errors, a chunked launch, the pipeline, and the sampler."""
import ctypes as C

import numpy as np
import pytest

from remixt_amd import posteriors, synthetic
from tests import helpers as H
from tests import span_twin
from tests.test_hip_region_events import LABELS, MASKS, Case
from tests.test_hip_sample_cn import GRIDS, _fitted, _model_state, _pipeline_case, _same_results

pytestmark = pytest.mark.gpu

WL, WR = 5, 18      # the second column group (right offsets 16 .. 18) is exercised at every state count
# none, loh, subclonal, state, total, (not_loh, total)
CONSTRAINTS = [(None, None), ('loh', None), ('subclonal', None), (None, 'state'), (None, 'total'), ('not_loh', 'total')]
# chains per fit of GRIDS, so that the longest chain has at least 20 model segments
CHAINS = {8: 2, 12: 2, 6: 1}


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


def _queries(anchors, constraints):
    return np.array([[n0, -1 if mk is None else MASKS.index(mk), -1 if lb is None else LABELS.index(lb), 0]
                     for n0 in anchors for (mk, lb) in constraints], dtype=np.int32)


def _raw(case, anchors, constraints=CONSTRAINTS, wl=WL, wr=WR, r0=None, nr=1):
    """(nr, anchors, constraints, wl + 1, wr + 1)"""
    out = case.b.region_span_raw(case.r if r0 is None else r0, nr, _queries(anchors, constraints), case.masks, case.labels, case.constrain, wl, wr)
    return out.reshape(nr, len(anchors), len(constraints), wl + 1, wr + 1)


def _extent_raw(case, anchors, constraints=CONSTRAINTS, wl=WL, wr=WR):
    out = case.b.region_extent_raw(case.r, 1, _queries(anchors, constraints), case.masks, case.labels, case.constrain, wl, wr)
    return out.reshape(len(anchors), len(constraints), wl + wr + 1)


def _breakend_adjacencies(case):
    inner = np.ones(case.N - 1, dtype=bool); inner[case.ce[:-1]] = False
    return np.flatnonzero(inner & (case.bidx[:-1] >= 0))


def _chain(case, n0):
    c = int(np.searchsorted(case.ce, n0, side='left'))
    return int(case.cs[c]), int(case.ce[c])


def _anchors(case):
    """The longest chain's first segment, a middle segment of it with at least WR segments to its right, and the two segments
    of a breakend adjacency."""
    c = int(np.argmax(case.ce - case.cs))
    c0, c1 = int(case.cs[c]), int(case.ce[c])
    assert c1 - c0 + 1 >= 20, 'the longest chain needs at least 20 model segments'
    mid = min((c0 + c1) // 2, c1 - WR)
    assert mid > c0 and c1 - mid >= WR
    be = _breakend_adjacencies(case)
    assert len(be), 'the case needs a breakend adjacency'
    return [c0, mid, int(be[0]), int(be[0]) + 1]


def _twin_tables(case, anchors, constraints=CONSTRAINTS, wl=WL, wr=WR):
    out = np.zeros((len(anchors), len(constraints), wl + 1, wr + 1))
    for i, n0 in enumerate(anchors):
        for j, (mk, lb) in enumerate(constraints):
            out[i, j] = span_twin.span(case.twin, n0, wl, wr, None if mk is None else case.mask_seg[mk],
                                       None if lb is None else case.label_seg[lb], case.constrain)
    return out


def _check(got, want, tag):
    """Finite entries within (a + c + 1) 1e-9 in log P (DESIGN 4.14's bound with steps = a + c), -inf entries -inf on both
    sides; prints the worst error relative to the bound and the lowest log P."""
    assert got.shape == want.shape
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), (tag, np.argwhere(np.isneginf(got) != np.isneginf(want))[:5])
    assert not np.isnan(got).any() and not np.isposinf(got).any()
    steps = np.arange(got.shape[-2])[:, None] + np.arange(got.shape[-1])[None, :]
    fin = np.isfinite(want)
    err = np.where(fin, np.abs(np.where(fin, got, 0.) - np.where(fin, want, 0.)), 0.) / ((steps + 1) * 1e-9)
    print('%s: %d finite entries, %d -inf, worst |d log P| / bound %.3e, lowest log P %.3f'
          % (tag, fin.sum(), (~fin).sum(), err.max(), want[fin].min() if fin.any() else np.nan))
    assert (err <= 1.).all(), (tag, np.argwhere(err > 1.)[:5], err.max())
    return err.max()


class SpanCase(Case):
    def __init__(self, m, **kw):
        Case.__init__(self, m, **kw)
        self.anchors = _anchors(self)
        self.want = _twin_tables(self, self.anchors)      # (computed once, shared by the tests of the grid)


@pytest.fixture(scope='module')
def cases(hip):
    return dict(((N, M, c), SpanCase(_fitted(hip, N, M, c, chains=CHAINS[c]))) for N, M, c in GRIDS)


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_twin(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    assert case.S == {8: 165, 12: 355, 6: 457}[max_cn] and case.S % 64
    assert (case.ce - case.cs + 1).max() >= 20
    b = case.b
    b.profile_reset(); b.profile_enable(1)
    got = _raw(case, case.anchors)[0]
    prof = b.profile(); b.profile_enable(0)
    assert prof['k_region_span'][1] == 1 and prof['k_region_span'][0] > 0
    # the second column group holds finite entries: the middle anchor has WR segments to its right
    rows = min(WL, case.anchors[1] - _chain(case, case.anchors[1])[0]) + 1
    assert rows >= 2 and np.isfinite(got[1, 0, :rows, 16:]).all()
    _check(got, case.want, 'S %d against the twin' % case.S)
    # the model-level form
    q = _queries(case.anchors, CONSTRAINTS[:3])
    one = case.m.model.region_span(q, case.masks, case.labels, case.constrain, WL, WR)
    assert one.shape == (len(q), WL + 1, WR + 1)
    assert np.array_equal(one, b.region_span_raw(case.r, 1, q, case.masks, case.labels, case.constrain, WL, WR)[0])


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_region_prob_and_extent(hip, cases, N, M, max_cn):
    """Every entry against k_region_prob on the same interval; row 0 and column 0 against k_region_extent."""
    case = cases[(N, M, max_cn)]
    got = _raw(case, case.anchors)[0]
    want = np.full(got.shape, -np.inf)
    runs, where = [], []
    for i, n0 in enumerate(case.anchors):
        c0, c1 = _chain(case, n0)
        for a in range(WL + 1):
            for c in range(WR + 1):
                if c0 <= n0 - a and n0 + c <= c1:
                    runs.append((n0 - a, n0 + c)); where.append((i, a, c))
    lp = case.raw(runs, CONSTRAINTS)[0]                   # (runs, constraints) from rmx_region_prob
    for (i, a, c), row in zip(where, lp):
        want[i, :, a, c] = row
    _check(got, want, 'S %d against k_region_prob' % case.S)
    ext = _extent_raw(case, case.anchors)
    _check(got[:, :, :1, :], ext[:, :, None, WL:], 'S %d row 0 against k_region_extent' % case.S)
    _check(got[:, :, :, :1], ext[:, :, WL::-1, None], 'S %d column 0 against k_region_extent' % case.S)


def test_identities(hip, cases):
    case = cases[GRIDS[0]]
    anchors = list(range(case.N))                         # every segment of the 165-state fit as anchor
    got = _raw(case, anchors)[0]
    for i, n0 in enumerate(anchors):
        c0, c1 = _chain(case, n0)
        inside = ((n0 - np.arange(WL + 1))[:, None] >= c0) & ((n0 + np.arange(WR + 1))[None, :] <= c1)
        # entries outside the chain are -inf, whatever the event
        assert np.isneginf(got[i][:, ~inside]).all(), n0
        # without mask and label every in-chain entry is log 1
        assert (np.abs(got[i, 0][inside]) <= 1e-12).all(), (n0, got[i, 0])
        t = got[i][:, :min(WL, n0 - c0) + 1, :min(WR, c1 - n0) + 1]
        assert not np.isnan(t).any() and (t <= 1e-12).all()
        # the table does not increase in a or in c; once -inf, always -inf further out
        with np.errstate(invalid='ignore'):
            assert (np.nan_to_num(np.diff(t, axis=1), nan=0., neginf=0.) <= 1e-12).all(), n0
            assert (np.nan_to_num(np.diff(t, axis=2), nan=0., neginf=0.) <= 1e-12).all(), n0
        assert (np.isneginf(t[:, :-1]) <= np.isneginf(t[:, 1:])).all() and (np.isneginf(t[:, :, :-1]) <= np.isneginf(t[:, :, 1:])).all()


def test_two_classes(hip):
    m, h, e = H.make_model(hip, N=40, M=3, max_cn=4, chains=2)
    M = 3
    classes, _ = m._state_tables(M)
    classes = np.repeat(classes[:1], 2, axis=0)
    classes[1, :, 0, :] = (1, 0)
    N = m.N1
    seg_class = (np.arange(N) % 2).astype(np.int32)                      # 0, 1, 0, 1, ...
    brk_states = m.create_brk_states(M, m.max_copy_number, m.max_copy_number_diff)
    b = hip.RemixtBatch(M, N, m.num_breakpoints, m.normal_contamination, classes, seg_class, brk_states, np.asarray(h, dtype=float)[None],
                        m.l1, m.x1[:, 2].copy(), m.x1[:, 0:2].copy(), m.is_telomere, m.breakpoint_idx, m.breakpoint_orient,
                        m.transition_log_prob, [m.divergence_weight])
    try:
        # (a normal row of (1, 0) makes LOH states whose allele likelihood is the reference's ValueError: total read counts alone)
        b.set_array(0, 'allele_likelihood_mask', np.zeros(N, dtype=np.int64))
        b.variational_update(2)
        case = Case(m, batch=b, r=0)
        loh = case.masks[:, MASKS.index('loh')]
        assert not loh[0].any() and loh[1].any()                         # the mask differs per class
        anchors = _anchors(case)
        _check(_raw(case, anchors)[0], _twin_tables(case, anchors), 'two classes')
        # (a kernel that took class 0's masks everywhere would call LOH impossible at the odd segments)
        odd = [n for n in range(1, N, 2) if case.constrain[n]]
        assert (_raw(case, odd, [('loh', None)], 0, 0)[0, :, 0, 0, 0] > -np.inf).any()
        even = [n for n in range(0, N, 2) if case.constrain[n]]
        assert np.isneginf(_raw(case, even, [('loh', None)], 0, 0)[0, :, 0, 0, 0]).all()
    finally:
        b.close()


def test_mixed_transition_model(hip):
    """The snapshot of the last update_p_cn under another transition_model than the current one, in both directions."""
    m = _fitted(hip, 40, 3, 4, seed=3, chains=2)
    T0 = np.array(m.model.log_transmat)
    m.model.transition_model = 1
    assert np.array_equal(np.array(m.model.log_transmat), T0)            # the snapshot stays the model-0 one
    case = Case(m)
    anchors = _anchors(case)
    _check(_raw(case, anchors)[0], _twin_tables(case, anchors), 'mixed model 0 -> 1')
    m2 = _fitted(hip, 40, 3, 4, seed=3, chains=2, transition_model=1)
    assert m2.model.transition_model == 1
    m2.model.transition_model = 0
    case2 = Case(m2)
    assert not np.array_equal(np.array(m2.model.log_transmat), T0)
    cons = [CONSTRAINTS[0], CONSTRAINTS[3], CONSTRAINTS[5]]
    anchors2 = _anchors(case2)
    _check(_raw(case2, anchors2, cons)[0], _twin_tables(case2, anchors2, cons), 'mixed model 1 -> 0')


def test_degenerate_windows(hip, cases):
    """wl = 0, wr = 0, both 0, wr = 15 and wr = 16 (one column group, and one column in the second), a chain of one segment."""
    case = cases[GRIDS[0]]
    full = _raw(case, case.anchors)[0]
    assert np.array_equal(_raw(case, case.anchors, wl=0, wr=WR)[0], full[..., :1, :])
    assert np.array_equal(_raw(case, case.anchors, wl=WL, wr=0)[0], full[..., :, :1])
    assert np.array_equal(_raw(case, case.anchors, wl=0, wr=0)[0], full[..., :1, :1])
    assert np.array_equal(_raw(case, case.anchors, wl=WL, wr=15)[0], full[..., :, :16])
    assert np.array_equal(_raw(case, case.anchors, wl=WL, wr=16)[0], full[..., :, :17])
    e = synthetic.make_experiment(30, num_clones=3, max_copy_number=3, num_chains=2, seed=1)
    k = 7
    e.adjacencies = set(a for a in e.adjacencies if a not in ((k - 1, k), (k, k + 1)))
    m, h, _ = H.make_model(hip, M=3, max_cn=3, experiment=e)
    H.attach(m, h)
    m.variational_update(); m.variational_update()
    one = Case(m)
    single = np.flatnonzero(one.cs == one.ce)
    assert len(single) == 1 and 0 < one.cs[single[0]] < one.N - 1
    n0 = int(one.cs[single[0]])
    assert m.seg_fwd_remap[k] == n0
    got = _raw(one, [n0], wl=3, wr=3)[0, 0]
    _check(got[None], _twin_tables(one, [n0], wl=3, wr=3), 'one-segment chain')
    assert np.isneginf(got[:, 1:, :]).all() and np.isneginf(got[:, :, 1:]).all() and (got[:, 0, 0] <= 0).all() and np.isfinite(got[0, 0, 0])
    # its neighbours' windows stop at it
    nb = _raw(one, [n0 - 1, n0 + 1], wl=3, wr=3)[0]
    assert np.isneginf(nb[0][:, :, 1:]).all() and np.isneginf(nb[1][:, 1:, :]).all() and np.isfinite(nb[0][0, :, 0]).all() and np.isfinite(nb[1][0, 0, :]).all()
    # the public form: anchors are experiment segments, the report holds no inserted segment
    s = m.event_span([k], 'total', 3)[0]
    assert s['right_segments'].tolist() == [k] and s['left_segments'].tolist() == [k] and not s['left_open'] and not s['right_open']
    assert abs(s['p_event'] - 1) <= 1e-12 and s['joint_pmf'].shape == (1, 1)
    assert np.abs(s['length_quantiles'] / m.l1[n0] - 1).max() <= 1e-12 and not s['length_censored'].any()


def test_invariance(hip):
    """An entry is bit-identical in any restart range, any batch of queries and any window that covers it."""
    from remixt_amd.restarts import RestartGroups, RestartSet
    e = synthetic.make_experiment(80, num_clones=3, max_copy_number=4, num_chains=3, seed=4)
    ps = synthetic.make_init_params(e, 4, 4)
    rs = RestartSet(e, ps, 4, num_clones=3, quiet=True, seeds=list(range(4)))
    rs.variational_update(2)
    b, m = rs.batch, rs.models[0]
    masks, labels = posteriors.event_tables(b.cn_classes)
    constrain = np.asarray(m.seg_is_original, dtype=np.uint8)
    q = np.array([[n0, mi, li, 0] for n0 in range(0, b.num_segments, 5) for mi, li in ((-1, -1), (1, -1), (-1, 1), (5, 2))], dtype=np.int32)
    call = lambda r0, nr, qq, wl=WL, wr=WR: b.region_span_raw(r0, nr, qq, masks, labels, constrain, wl, wr)
    full = call(0, 4, q)
    assert full.shape == (4, len(q), WL + 1, WR + 1) and not np.array_equal(full[0], full[1]) and not np.isnan(full).any()
    for r in range(4):
        assert np.array_equal(call(r, 1, q)[0], full[r])
    assert np.array_equal(call(1, 2, q), full[1:3])
    for i in range(0, len(q), 5):
        assert np.array_equal(call(0, 4, q[i:i + 1])[:, 0], full[:, i])
    assert np.array_equal(call(0, 4, q[::-1].copy()), full[:, ::-1])
    for wl, wr in ((0, 18), (5, 0), (3, 7), (9, 40)):
        other = call(0, 4, q, wl, wr)
        lo, hi = min(wl, WL), min(wr, WR)
        assert np.array_equal(other[:, :, :lo + 1, :hi + 1], full[:, :, :lo + 1, :hi + 1]), (wl, wr)
    # the public forms: one restart of a set, and groups against one group
    anchors = [0, 11, 40, 79]
    same = lambda a, c: sorted(a) == sorted(c) and all(np.array_equal(a[k], c[k], equal_nan=True) for k in a if k != 'length_cdf') and \
        all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a['length_cdf']([1e4, 1e6]), c['length_cdf']([1e4, 1e6])))
    per_set = rs.event_span(anchors, ('not_loh', 'total'), (WL, WR))
    one = rs.models[2].event_span(anchors, ('not_loh', 'total'), (WL, WR))
    assert len(per_set) == 4 and len(per_set[2]) == len(anchors)
    assert all(same(a, c) for a, c in zip(per_set[2], one))
    rs.close()
    groups = RestartGroups(e, ps, 4, groups=2, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    single = RestartGroups(e, ps, 4, groups=1, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    for g in (groups, single):
        g.variational_update(2)
    x, y = groups.event_span(anchors, 'state', (WL, WR)), single.event_span(anchors, 'state', (WL, WR))
    assert len(x) == len(y) == 4
    for r in range(4):
        assert all(same(a, c) for a, c in zip(x[r], y[r]))
    groups.close(); single.close()


def test_no_side_effects(hip):
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    before = _model_state(m1)
    out = m1.event_span([0, 20, 49], 'total', (WL, WR))
    assert len(out) == 3 and all(0 <= s['p_event'] <= 1 for s in out)
    after = _model_state(m1)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    # a fit continued after the call equals one without it
    for m in (m1, m2):
        m.variational_update()
        m.variational_update()
    s1, s2 = _model_state(m1), _model_state(m2)
    for k in s1:
        assert np.array_equal(s1[k], s2[k], equal_nan=True), k
    assert m1.model.calculate_elbo() == m2.model.calculate_elbo()


def _c_call(b, r, nr, q, masks, labels, constrain, wl, wr, out, null=None):
    """rmx_region_span through ctypes with the caller's output buffer: the return code."""
    dp, ip, u8p, i16p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int16)
    q = np.ascontiguousarray(q, dtype=np.int32).reshape(-1, 4)
    masks, labels = np.ascontiguousarray(masks, dtype=np.uint8), np.ascontiguousarray(labels, dtype=np.int16)
    constrain = np.ascontiguousarray(constrain, dtype=np.uint8)
    return b._lib.rmx_region_span(b._handle, r, nr, len(q), q.ctypes.data_as(ip) if len(q) else ip(), masks.shape[1],
                                  u8p() if null == 'masks' else masks.ctypes.data_as(u8p), labels.shape[1],
                                  i16p() if null == 'labels' else labels.ctypes.data_as(i16p), constrain.ctypes.data_as(u8p), wl, wr,
                                  dp() if null == 'out' else out.ctypes.data_as(dp))


def test_errors(hip):
    import re
    from remixt_amd import bpmodel
    m, h, e = H.make_model(hip, N=30, M=3, max_cn=3)
    H.attach(m, h)
    b, r = m.model._batch, m.model._r
    masks, labels = posteriors.event_tables(b.cn_classes)
    N = b.num_segments
    constrain = np.ones(N, dtype=np.uint8)
    ok = [[3, 0, 0, 0]]
    out = np.full(256, -7.)
    # before update_p_cn: RMX_EVALUE with the restart listed
    assert _c_call(b, r, 1, ok, masks, labels, constrain, 2, 2, out) == bpmodel.RMX_EVALUE and (out == -7.).all()
    with pytest.raises(ValueError, match='update_p_cn'):
        b.region_span_raw(r, 1, ok, masks, labels, constrain, 2, 2)
    assert bpmodel.last_error_restarts() == [r]
    with pytest.raises(ValueError, match='update_p_cn'):
        m.event_span([3], 'loh', 2)
    m.variational_update()
    b.profile_reset(); b.profile_enable(1)
    assert b.region_span_raw(r, 1, ok, masks, labels, constrain, 2, 3).shape == (1, 1, 3, 4)
    launches = b.profile()['k_region_span'][1]
    assert launches == 1
    bad = [((r, 1), ok + [[-1, 0, 0, 0]], 2, 2, None, 'anchor'), ((r, 1), ok + [[N, 0, 0, 0]], 2, 2, None, 'anchor'),
           ((r, 1), ok + [[3, len(MASKS), 0, 0]], 2, 2, None, 'mask index'), ((r, 1), ok + [[3, -2, 0, 0]], 2, 2, None, 'mask index'),
           ((r, 1), ok + [[3, 0, len(LABELS), 0]], 2, 2, None, 'label index'), ((r, 1), ok + [[3, 0, -2, 0]], 2, 2, None, 'label index'),
           ((r, 1), ok + [[3, 0, 0, 1]], 2, 2, None, 'fourth field'), ((r, 1), ok + [[3, 0, 0, -1]], 2, 2, None, 'fourth field'),
           ((r, 1), ok, -1, 2, None, 'window'), ((r, 1), ok, 2, -1, None, 'window'), ((r, 1), ok, 127, 128, None, 'window'),     # one past the cap
           ((r, 1), ok, 128, 127, None, 'window'), ((r, 1), ok, 0, 16384, None, 'window'),
           ((r, 1), ok, 2 ** 31 - 1, 2 ** 31 - 1, None, 'window'), ((r, 1), [], 2, 2, None, 'no queries'), ((r, 1), ok, 2, 2, 'masks', 'tables'),
           ((r, 1), ok, 2, 2, 'labels', 'tables'), ((r + 1, 1), ok, 2, 2, None, 'restart range'), ((-1, 1), ok, 2, 2, None, 'restart range'),
           ((r, 0), ok, 2, 2, None, 'restart range')]
    for (r0, nr), q, wl, wr, null, text in bad:
        assert _c_call(b, r0, nr, q, masks, labels, constrain, wl, wr, out, null) == bpmodel.RMX_EARG, (q, wl, wr, null, text)
        assert (out == -7.).all(), (q, wl, wr, null, text)                 # the output buffer is untouched
        assert re.search(text, hip._lib.load().rmx_last_error().decode()), (text, hip._lib.load().rmx_last_error())
        assert bpmodel.last_error_restarts() == []
        assert b.profile()['k_region_span'][1] == launches, (q, wl, wr)    # nothing was launched
    assert _c_call(b, r, 1, ok, masks, labels, constrain, 2, 2, out, 'out') == bpmodel.RMX_EARG
    wide = np.full(16384, -7.)
    okw = [[3, -1, 0, 0]]                                                 # (an event with mass: `loh` has none under a normal clone of (1, 1))
    assert _c_call(b, r, 1, okw, masks, labels, constrain, 127, 127, wide) == 0     # the widest square window
    wide = wide.reshape(128, 128)
    c0, c1 = [(int(s), int(t)) for s, t in zip(*posteriors.chains_from_telomeres(np.asarray(m.is_telomere))) if s <= 3 <= t][0]
    inside = ((3 - np.arange(128))[:, None] >= c0) & ((3 + np.arange(128))[None, :] <= c1)
    assert np.isneginf(wide[~inside]).all() and not np.isnan(wide).any() and np.isfinite(wide[0, 0])
    assert np.array_equal(wide[:3, :4], b.region_span_raw(r, 1, okw, masks, labels, constrain, 2, 3)[0, 0])
    b.profile_enable(0)
    with pytest.raises(ValueError, match='^bad argument: .*mask index'):      # an index without a table
        b.region_span_raw(r, 1, ok, None, labels, constrain, 2, 2)
    with pytest.raises(ValueError, match='^bad argument: .*window'):
        b.region_span_raw(r, 1, ok, masks, labels, constrain, 4000, 4000)
    for kw in (dict(queries=[[0, 1, 0]]), dict(masks=masks[:, :, :-1]), dict(labels=labels[:1, :, :-1]), dict(constrain=np.ones(N + 1))):
        args = dict(queries=ok, masks=masks, labels=labels, constrain=None); args.update(kw)
        with pytest.raises(ValueError, match='must have shape'):
            b.region_span_raw(r, 1, wl=2, wr=2, **args)
    for bad_call in (lambda: m.event_span([30], 'loh'), lambda: m.event_span([3], 'nothing'), lambda: m.event_span([3], 'loh', -1),
                     lambda: m.event_span([3], 'loh', 128)):
        with pytest.raises(ValueError):
            bad_call()


def test_chunked_launch(hip, cases):
    """16 384 entries per query -- the window (7, 2047): 128 column groups -- and enough copies of three queries to need two
    launches."""
    case = cases[GRIDS[0]]
    b = case.b
    wl, wr = 7, 2047
    per = (wl + 1) * (wr + 1)
    assert per == 16384
    reps = (64 << 20) // (per * 8 + 16) + 2
    few = _queries(case.anchors[:3], [('not_loh', 'total')])
    many = np.tile(few, ((reps + 2) // 3, 1))
    b.profile_reset(); b.profile_enable(1)
    big = b.region_span_raw(case.r, 1, many, case.masks, case.labels, case.constrain, wl, wr)
    launches = b.profile()['k_region_span'][1]; b.profile_enable(0)
    assert launches >= 2 and big.shape == (1, len(many), wl + 1, wr + 1)
    small = b.region_span_raw(case.r, 1, few, case.masks, case.labels, case.constrain, wl, wr)
    assert np.array_equal(big[0].reshape(-1, 3, per), np.broadcast_to(small[0].reshape(3, per), (len(many) // 3, 3, per)))
    # the window covers every chain whole to the right: the narrow window's entries, and -inf everywhere outside the chain
    narrow = _raw(case, case.anchors[:3], [('not_loh', 'total')])[0, :, 0]
    assert np.array_equal(small[0][:, :WL + 1, :WR + 1], narrow)
    for i, n0 in enumerate(case.anchors[:3]):
        c0, c1 = _chain(case, n0)
        inside = ((n0 - np.arange(wl + 1))[:, None] >= c0) & ((n0 + np.arange(wr + 1))[None, :] <= c1)
        assert np.isneginf(small[0, i][~inside]).all() and not np.isnan(small[0, i]).any() and np.isfinite(small[0, i, 0, 0])


def test_pipeline_cn_event_lengths(hip, tmp_path):
    from remixt_amd import restarts, workflow
    from remixt_amd.analysis import pipeline
    from remixt_amd.restarts import RestartSet
    import pickle
    e, config, init_params = _pipeline_case()
    ids = sorted(init_params)
    seeds = [100 + i for i in ids]
    extents = [('run', 77, 'state'), ('tot', 300, 'total'), ('both', 150, ('not_loh', 'total')), ('sub', 5, 'not_subclonal')]
    names = [x[0] for x in extents]
    edges = [2e5, 5e6]
    on_cfg = dict(config, cn_event_extents=extents, cn_extent_window=20, cn_event_lengths=True, cn_event_length_edges=edges)
    base = pipeline.fit_restarts(e, init_params, dict(config, cn_event_extents=extents, cn_extent_window=20), seeds=seeds, groups=1)
    off = pipeline.fit_restarts(e, init_params, dict(config, cn_event_extents=extents, cn_extent_window=20, cn_event_lengths=False, cn_event_length_edges=edges),
                                seeds=seeds, groups=1)
    on = pipeline.fit_restarts(e, init_params, on_cfg, seeds=seeds, groups=1)
    # off: nothing of it in the results (they equal the ones without the option); on: the same results plus event_lengths
    assert not any('event_lengths' in res for res in base.values()) and not any('event_lengths' in res for res in off.values())
    plain = lambda results: dict((i, dict((k, v) for k, v in res.items() if k not in ('event_lengths', 'event_extents'))) for i, res in results.items())
    _same_results(plain(base), plain(off))
    _same_results(plain(base), plain(on))
    for i in ids:
        assert sorted(base[i]) == sorted(off[i]) == sorted(k for k in on[i] if k != 'event_lengths')
        for k in posteriors.EXTENT_ARRAYS:
            assert np.array_equal(base[i]['event_extents'][k], on[i]['event_extents'][k]) and np.array_equal(base[i]['event_extents'][k], off[i]['event_extents'][k]), k
    # recomputation from the same fit
    rs = RestartSet(e, [init_params[i] for i in ids], 4, num_clones=3, quiet=True, seeds=seeds, **pipeline._model_kwargs(e, config))
    rs.fit(config['num_em_iter'], config['num_update_iter'])
    want = [rs.event_span([seg], ev, 20) for _, seg, ev in extents]      # [entry][restart][0]
    rs.close()
    keys = posteriors.SPAN_ARRAYS + posteriors.SPAN_EDGE_ARRAYS
    for j, i in enumerate(ids):
        ln = on[i]['event_lengths']
        assert ln['names'] == names and sorted(ln) == sorted(keys + ('names',))
        for a in range(len(extents)):
            c = posteriors.compact_spans([want[a][j][0]], edges)
            for k in keys:
                assert ln[k].shape == ((len(extents),) if k in posteriors.SPAN_ARRAYS else (len(extents), 2))
                assert np.array_equal(ln[k][a], c[k][0], equal_nan=True), (i, a, k)
            if on[i]['event_extents']['p_event'][a] > 0:
                assert 0 < ln['length_q05'][a] <= ln['length_q50'][a] <= ln['length_q95'][a]
                assert (ln['p_length_le'][a] >= 0).all() and (np.diff(ln['p_length_le'][a]) >= 0).all()
                assert (ln['p_length_le'][a] + ln['p_length_undetermined'][a] <= 1 + 1e-12).all()
    one = pipeline.fit(e, init_params[ids[1]], on_cfg, quiet=True, init_id=ids[1])
    assert one['event_lengths']['names'] == names and one['event_lengths']['p_length_le'].shape == (len(extents), 2)
    # the distributed form: the arrays through the record
    dist = restarts.fit_restarts_distributed(e, [init_params[i] for i in ids], 4, num_clones=3, num_em_iter=config['num_em_iter'],
                                             num_update_iter=config['num_update_iter'], seeds=seeds, quiet=True, cn_event_extents=extents,
                                             cn_extent_window=20, cn_event_lengths=True, cn_event_length_edges=edges, **pipeline._model_kwargs(e, config))
    for j, i in enumerate(ids):
        assert dist[j]['event_lengths']['names'] == names
        for k in keys:
            assert dist[j]['event_lengths'][k].dtype == on[i]['event_lengths'][k].dtype and dist[j]['event_lengths'][k].shape == on[i]['event_lengths'][k].shape
    # the workflow (fit_restarts_distributed + collate): the arrays in the store
    exp_file = str(tmp_path / 'experiment.pickle')
    with open(exp_file, 'wb') as f:
        pickle.dump(e, f)
    workflow.fit_model(exp_file, str(tmp_path / 'r.store'), on_cfg, None, seeds=seeds)
    with pipeline._Store(str(tmp_path / 'r.store'), 'r') as st:
        for i in sorted(st['stats']['init_id']):
            assert list(st['solutions/solution_%d/span_names' % i]) == names
            for k in keys:
                v = np.asarray(st['solutions/solution_%d/span_%s' % (i, k)])
                assert np.array_equal(v, dist[ids.index(i)]['event_lengths'][k], equal_nan=True), (i, k)
    workflow.fit_model(exp_file, str(tmp_path / 'r0.store'), dict(config, cn_event_extents=extents, cn_extent_window=20), None, seeds=seeds)
    with pipeline._Store(str(tmp_path / 'r0.store'), 'r') as st:
        assert not any('span_' in k for k in st.keys())


def test_against_the_sampler(hip):
    """4 096 sampled paths: the empirical joint pmf of (left end, right end) around two anchors within 4 binomial SDs of the
    exact one wherever the exact mass is above 1 %; at least 5 such cells."""
    from tests.test_hip_posterior_summary import _fitted as fitted_masked
    m = fitted_masked(hip, 30, 3, 8, sweeps=3, masked=True, seed=1)      # (read counts masked out: events of intermediate probability)
    case = Case(m)
    assert case.S == 165
    K = 4096
    st = case.b.sample_states(case.r, 1, K, [99]).astype(np.int64)[0]
    fwd = np.asarray(m.seg_fwd_remap)
    # (in this fit the runs that end inside a window are the subclonal / not subclonal ones; label changes are rare)
    events = (('subclonal', None), ('not_subclonal', None), ('not_subclonal', 'state'), 'state')
    # the two anchors whose exact joint pmfs spread over the most cells (chosen from the exact tables alone)
    spread = np.zeros(len(fwd), dtype=int)
    for event in events:
        spread += [int(((s['joint_pmf'] > 0.01) & (s['joint_pmf'] < 0.99)).sum()) for s in m.event_span(np.arange(len(fwd)), event, (6, 6))]
    anchors = sorted(int(a) for a in np.argsort(-spread, kind='stable')[:2])
    print('anchors %s: %s cells of intermediate exact mass over the events' % (anchors, spread[anchors].tolist()))
    cells = 0
    for event in events:
        mi, li = posteriors.parse_event(event)
        mk = None if mi < 0 else case.mask_seg[MASKS[mi]]
        lb = None if li < 0 else case.label_seg[LABELS[li]]
        for a, s in zip(anchors, m.event_span(anchors, event, (6, 6))):
            n0 = int(fwd[a])
            c0, c1 = _chain(case, n0)
            ok_at = lambda n: np.ones(K, dtype=bool) if (mk is None or not case.constrain[n]) else mk[n, st[:, n]]
            # per sample: the farthest model segment the event reaches on either side (within the chain; -1: not at the anchor)
            reach = {}
            for side, step in (('right', 1), ('left', -1)):
                alive = ok_at(n0)
                far = np.where(alive, n0, -1)
                n = n0
                while c0 <= n + step <= c1:
                    if lb is not None:
                        alive = alive & (lb[n, st[:, n]] == lb[n + step, st[:, n + step]])
                    n += step
                    alive = alive & ok_at(n)
                    far = np.where(alive, n, far)
                reach[side] = far
            # the event over [l, r] holds iff it reaches l on the left and r on the right (both walks start from the anchor)
            L, R = fwd[s['left_segments']], fwd[s['right_segments']]
            pmf = s['joint_pmf']
            at = reach['right'] >= 0
            for i in range(len(L)):
                # left end in cell i: reaches L[i] but not the next original segment to the left (or anything beyond, in the lump)
                hl = at & (reach['left'] <= L[i]) & ((reach['left'] > L[i + 1]) if i + 1 < len(L) else True)
                for j in range(len(R)):
                    hr = (reach['right'] >= R[j]) & ((reach['right'] < R[j + 1]) if j + 1 < len(R) else True)
                    P = pmf[i, j]
                    if P > 0.01:
                        cells += P < 0.99
                        freq = (hl & hr).mean()
                        assert abs(freq - P) <= 4 * np.sqrt(P * (1 - min(P, 1.)) / K), (event, a, i, j, freq, P)
    print('%d cells of intermediate exact mass' % cells)
    assert cells >= 5
