"""Region event extents on the device (rmx_region_extent / k_region_extent): against the numpy twin (RegionTwin.logprob per
nested interval) on the read-back framelogprob / log_transmat, against rmx_region_prob on the same intervals, the exact
identities, two state classes, the mixed-model state, degenerate windows, bit identity across restart ranges, query
batches and windows, no side effects on the model, errors, a chunked launch, the pipeline, and the sampler."""
import ctypes as C

import numpy as np
import pytest

from remixt_amd import posteriors, synthetic
from tests import extent_twin
from tests import helpers as H
from tests.test_hip_region_events import CONSTRAINTS, LABELS, MASKS, Case
from tests.test_hip_sample_cn import GRIDS, _fitted, _model_state, _pipeline_case, _same_results

pytestmark = pytest.mark.gpu

U = 2. ** -53
W = 12      # window width on each side


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


def _queries(anchors, constraints):
    return np.array([[n0, -1 if mk is None else MASKS.index(mk), -1 if lb is None else LABELS.index(lb), 0]
                     for n0 in anchors for (mk, lb) in constraints], dtype=np.int32)


def _raw(case, anchors, constraints=CONSTRAINTS, wl=W, wr=W, r0=None, nr=1):
    """(nr, anchors, constraints, wl + wr + 1)"""
    out = case.b.region_extent_raw(case.r if r0 is None else r0, nr, _queries(anchors, constraints), case.masks, case.labels, case.constrain, wl, wr)
    return out.reshape(nr, len(anchors), len(constraints), wl + wr + 1)


def _breakend_adjacencies(case):
    inner = np.ones(case.N - 1, dtype=bool); inner[case.ce[:-1]] = False
    return np.flatnonzero(inner & (case.bidx[:-1] >= 0))


def _anchors(case):
    """A chain's first, last and a middle segment, and the two segments of a breakend adjacency."""
    c = int(np.argmax(case.ce - case.cs))
    be = _breakend_adjacencies(case)
    assert len(be), 'the case needs a breakend adjacency'
    return [int(case.cs[c]), int(case.ce[c]), int((case.cs[c] + case.ce[c]) // 2), int(be[0]), int(be[0]) + 1]


def _chain(case, n0):
    c = int(np.searchsorted(case.ce, n0, side='left'))
    return int(case.cs[c]), int(case.ce[c])


def _twin_rows(case, anchors, constraints=CONSTRAINTS, wl=W, wr=W):
    out = np.zeros((len(anchors), len(constraints), wl + wr + 1))
    for i, n0 in enumerate(anchors):
        for j, (mk, lb) in enumerate(constraints):
            out[i, j] = extent_twin.extent(case.twin, n0, wl, wr, None if mk is None else case.mask_seg[mk],
                                           None if lb is None else case.label_seg[lb], case.constrain)
    return out


def _check_rows(got, want, tag, wl=W):
    """Finite slots within (steps + 1) 1e-9 in log P, -inf slots -inf on both sides; the worst error relative to the bound."""
    assert got.shape == want.shape
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), (tag, np.argwhere(np.isneginf(got) != np.isneginf(want))[:5])
    assert not np.isnan(got).any() and not np.isposinf(got).any()
    steps = np.abs(np.arange(got.shape[-1]) - wl)
    fin = np.isfinite(want)
    err = np.where(fin, np.abs(np.where(fin, got, 0.) - np.where(fin, want, 0.)), 0.) / ((steps + 1) * 1e-9)
    print('%s: %d finite slots, %d -inf, worst |d log P| / bound %.3e, lowest log P %.3f' % (tag, fin.sum(), (~fin).sum(), err.max(), want[fin].min()))
    assert (err <= 1.).all(), (tag, np.argwhere(err > 1.)[:5], err.max())
    return err.max()


class ExtentCase(Case):
    def __init__(self, m, **kw):
        Case.__init__(self, m, **kw)
        self.anchors = _anchors(self)
        self.want = _twin_rows(self, self.anchors)      # (computed once, shared by the tests of the grid)


@pytest.fixture(scope='module')
def cases(hip):
    return dict(((N, M, c), ExtentCase(_fitted(hip, N, M, c))) for N, M, c in GRIDS)


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_twin(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    assert case.S == {8: 165, 12: 355, 6: 457}[max_cn] and case.S % 64
    be = _breakend_adjacencies(case)
    # at least one window crosses a breakend adjacency: the anchors on either side of one do, in both directions
    crossing = [(n0, n) for n0 in case.anchors for n in be if _chain(case, n0) == _chain(case, n) and (n0 - W <= n < n0 or n0 <= n < n0 + W)]
    assert crossing and (case.anchors[3], be[0]) in crossing and (case.anchors[4], be[0]) in crossing
    b = case.b
    b.profile_reset(); b.profile_enable(1)
    got = _raw(case, case.anchors)[0]
    prof = b.profile(); b.profile_enable(0)
    assert prof['k_region_extent'][1] == 1 and prof['k_region_extent'][0] > 0
    _check_rows(got, case.want, 'S %d against the twin' % case.S)
    # the model-level form
    q = _queries(case.anchors, CONSTRAINTS[:3])
    one = case.m.model.region_extent(q, case.masks, case.labels, case.constrain, W, W)
    assert one.shape == (len(q), 2 * W + 1) and np.array_equal(one, b.region_extent_raw(case.r, 1, q, case.masks, case.labels, case.constrain, W, W)[0])


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_region_prob(hip, cases, N, M, max_cn):
    """Every slot against k_region_prob on the same interval.  The left walk runs k_region_prob's start and step with the
    same sums in the same order: where the mask binds at the anchor (both then start from the same log Z) the left slots
    are equal to the last bit."""
    case = cases[(N, M, max_cn)]
    got = _raw(case, case.anchors)[0]
    want = np.full(got.shape, -np.inf)
    runs, where = [], []
    for i, n0 in enumerate(case.anchors):
        c0, c1 = _chain(case, n0)
        for k in range(2 * W + 1):
            n = n0 - W + k
            if c0 <= n <= c1:
                runs.append((min(n, n0), max(n, n0))); where.append((i, k))
    lp = case.raw(runs)[0]                                # (runs, constraints) from rmx_region_prob
    for (i, k), row in zip(where, lp):
        want[i, :, k] = row
    _check_rows(got, want, 'S %d against k_region_prob' % case.S)
    bound = [(i, j) for i, n0 in enumerate(case.anchors) if case.constrain[n0] for j, (mk, lb) in enumerate(CONSTRAINTS) if mk is not None]
    assert bound
    for i, j in bound:
        left = (got[i, j, :W], want[i, j, :W])
        print('anchor %d constraint %s: %d left slots differ from k_region_prob' % (case.anchors[i], CONSTRAINTS[j], (left[0] != left[1]).sum()))
        assert np.array_equal(*left), (case.anchors[i], CONSTRAINTS[j], left)


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_identities(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    b, S = case.b, case.S
    anchors = list(range(case.N))
    got = _raw(case, anchors)[0]                          # every segment as anchor
    for i, n0 in enumerate(anchors):
        c0, c1 = _chain(case, n0)
        n = n0 - W + np.arange(2 * W + 1)
        inside = (n >= c0) & (n <= c1)
        # slots outside the chain are -inf, whatever the event
        assert np.isneginf(got[i][:, ~inside]).all(), n0
        # without mask and label every in-chain slot is log 1
        assert (np.abs(got[i, 0, inside]) <= 1e-12).all(), (n0, got[i, 0])
        # the curves do not increase away from the anchor
        with np.errstate(invalid='ignore'):
            right = got[i][:, W:][:, inside[W:]]
            left = got[i][:, :W + 1][:, inside[:W + 1]]
            assert (np.nan_to_num(np.diff(right, axis=1), nan=0., neginf=0.) <= 1e-12).all(), n0
            assert (np.nan_to_num(np.diff(left, axis=1), nan=0., posinf=0.) >= -1e-12).all(), n0
        # (once -inf, always -inf further out)
        assert (np.isneginf(right[:, :-1]) <= np.isneginf(right[:, 1:])).all() and (np.isneginf(left[:, 1:]) <= np.isneginf(left[:, :-1])).all()
    # slot wl is the mask's row sum of the marginals, as rmx_posterior_summary projects them.  Both are sums of S products
    # in their own order: (S + 4) 2^-53 relative each, and what a float64 logarithm carries of log P (3 |log P| 2^-53)
    weights = np.ascontiguousarray(np.transpose(case.masks, (0, 2, 1)).astype(float))          # (C, S, masks)
    proj = b.posterior_summary_raw(case.r, 1, weights=weights, want_stats=False, want_argmax=False)[0][0]
    for j, (mk, lb) in enumerate(CONSTRAINTS):
        slot = got[:, j, W]
        if mk is None:
            assert (slot == 0).all(), (mk, lb)
            continue
        want = np.where(case.constrain, proj[:, MASKS.index(mk)], 1.)
        assert (slot[~case.constrain] == 0).all()
        assert np.array_equal(np.isneginf(slot), want == 0), mk
        ok = want > 0
        tol = (2 * (S + 4) + 3 * np.abs(np.log(want[ok]))) * U
        assert (np.abs(np.exp(slot[ok]) / want[ok] - 1) <= tol).all(), (mk, np.abs(np.exp(slot[ok]) / want[ok] - 1).max())


def test_two_classes(hip):
    m, h, e = H.make_model(hip, N=40, M=3, max_cn=4, chains=3)
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
        got = _raw(case, anchors)[0]
        _check_rows(got, _twin_rows(case, anchors), 'two classes')
        # (a kernel that took class 0's masks everywhere would call LOH impossible at the odd segments)
        odd = [n for n in range(1, N, 2) if case.constrain[n]]
        lp = _raw(case, odd, [('loh', None)], 0, 0)[0, :, 0, 0]
        assert (lp > -np.inf).any()
        even = [n for n in range(0, N, 2) if case.constrain[n]]
        assert np.isneginf(_raw(case, even, [('loh', None)], 0, 0)[0, :, 0, 0]).all()
    finally:
        b.close()


def test_mixed_transition_model(hip):
    """The snapshot of the last update_p_cn under another transition_model than the current one, in both directions."""
    m = _fitted(hip, 40, 3, 4, seed=3)
    T0 = np.array(m.model.log_transmat)
    m.model.transition_model = 1
    assert np.array_equal(np.array(m.model.log_transmat), T0)            # the snapshot stays the model-0 one
    case = Case(m)
    anchors = _anchors(case)
    _check_rows(_raw(case, anchors)[0], _twin_rows(case, anchors), 'mixed model 0 -> 1')
    m2 = _fitted(hip, 40, 3, 4, seed=3, transition_model=1)
    assert m2.model.transition_model == 1
    m2.model.transition_model = 0
    case2 = Case(m2)
    assert not np.array_equal(np.array(m2.model.log_transmat), T0)
    cons = CONSTRAINTS[:1] + CONSTRAINTS[7:]
    anchors2 = _anchors(case2)
    _check_rows(_raw(case2, anchors2, cons)[0], _twin_rows(case2, anchors2, cons), 'mixed model 1 -> 0')


def test_degenerate_windows(hip, cases):
    """wl = 0, wr = 0, both 0, and a chain of one segment."""
    case = cases[GRIDS[0]]
    full = _raw(case, case.anchors)[0]
    assert np.array_equal(_raw(case, case.anchors, wl=0, wr=W)[0], full[..., W:])
    assert np.array_equal(_raw(case, case.anchors, wl=W, wr=0)[0], full[..., :W + 1])
    assert np.array_equal(_raw(case, case.anchors, wl=0, wr=0)[0], full[..., W:W + 1])
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
    want = _twin_rows(one, [n0], wl=3, wr=3)[0]
    _check_rows(got[None], want[None], 'one-segment chain', wl=3)
    assert np.isneginf(got[:, :3]).all() and np.isneginf(got[:, 4:]).all() and (got[:, 3] <= 0).all() and np.isfinite(got[0, 3])
    # its neighbours' windows stop at it
    nb = _raw(one, [n0 - 1, n0 + 1], wl=3, wr=3)[0]
    assert np.isneginf(nb[0][:, 4:]).all() and np.isneginf(nb[1][:, :3]).all() and np.isfinite(nb[0][0, :4]).all() and np.isfinite(nb[1][0, 3:]).all()
    # the public form: anchors are experiment segments, the report holds no inserted segment
    s = m.event_extent([k], 'total', 3)[0]
    assert s['right_segments'].tolist() == [k] and s['left_segments'].tolist() == [k] and s['right_quantiles'].tolist() == [k] * 3
    assert not s['right_censored'].any() and not s['left_censored'].any() and abs(s['p_event'] - 1) <= 1e-12


def test_invariance(hip):
    """A (restart, query) slot is bit-identical in any restart range, any batch of queries and any window that covers it."""
    from remixt_amd.restarts import RestartGroups, RestartSet
    e = synthetic.make_experiment(80, num_clones=3, max_copy_number=4, num_chains=3, seed=4)
    ps = synthetic.make_init_params(e, 4, 4)
    rs = RestartSet(e, ps, 4, num_clones=3, quiet=True, seeds=list(range(4)))
    rs.variational_update(2)
    b, m = rs.batch, rs.models[0]
    masks, labels = posteriors.event_tables(b.cn_classes)
    constrain = np.asarray(m.seg_is_original, dtype=np.uint8)
    q = np.array([[n0, mi, li, 0] for n0 in range(0, b.num_segments, 5) for mi, li in ((-1, -1), (1, -1), (-1, 1), (5, 2))], dtype=np.int32)
    call = lambda r0, nr, qq, wl=W, wr=W: b.region_extent_raw(r0, nr, qq, masks, labels, constrain, wl, wr)
    full = call(0, 4, q)
    assert full.shape == (4, len(q), 2 * W + 1) and not np.array_equal(full[0], full[1]) and not np.isnan(full).any()
    for r in range(4):
        assert np.array_equal(call(r, 1, q)[0], full[r])
    assert np.array_equal(call(1, 2, q), full[1:3])
    for i in range(0, len(q), 5):
        assert np.array_equal(call(0, 4, q[i:i + 1])[:, 0], full[:, i])
    assert np.array_equal(call(0, 4, q[::-1].copy()), full[:, ::-1])
    for wl, wr in ((0, W), (W, 0), (3, 7), (W + 9, W + 20), (0, 0)):
        other = call(0, 4, q, wl, wr)
        lo, hi = min(wl, W), min(wr, W)
        assert np.array_equal(other[:, :, wl - lo:wl + hi + 1], full[:, :, W - lo:W + hi + 1]), (wl, wr)
    # the public forms: one restart of a set, and groups against one group
    anchors = [0, 11, 40, 79]
    per_set = rs.event_extent(anchors, ('not_loh', 'total'), W)
    one = rs.models[2].event_extent(anchors, ('not_loh', 'total'), W)
    assert len(per_set) == 4 and len(per_set[2]) == len(anchors)
    for a, c in zip(per_set[2], one):
        assert sorted(a) == sorted(c) and all(np.array_equal(a[k], c[k], equal_nan=True) for k in a)
    rs.close()
    groups = RestartGroups(e, ps, 4, groups=2, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    single = RestartGroups(e, ps, 4, groups=1, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    for g in (groups, single):
        g.variational_update(2)
    x, y = groups.event_extent(anchors, 'state', W), single.event_extent(anchors, 'state', W)
    assert len(x) == len(y) == 4
    for r in range(4):
        for a, c in zip(x[r], y[r]):
            assert all(np.array_equal(a[k], c[k], equal_nan=True) for k in a)
    groups.close(); single.close()


def test_no_side_effects(hip):
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    before = _model_state(m1)
    out = m1.event_extent([0, 20, 49], 'total', W)
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
    """rmx_region_extent through ctypes with the caller's output buffer: the return code."""
    dp, ip, u8p, i16p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int16)
    q = np.ascontiguousarray(q, dtype=np.int32).reshape(-1, 4)
    masks, labels = np.ascontiguousarray(masks, dtype=np.uint8), np.ascontiguousarray(labels, dtype=np.int16)
    constrain = np.ascontiguousarray(constrain, dtype=np.uint8)
    return b._lib.rmx_region_extent(b._handle, r, nr, len(q), q.ctypes.data_as(ip) if len(q) else ip(), masks.shape[1],
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
        b.region_extent_raw(r, 1, ok, masks, labels, constrain, 2, 2)
    assert bpmodel.last_error_restarts() == [r]
    with pytest.raises(ValueError, match='update_p_cn'):
        m.event_extent([3], 'loh', 2)
    m.variational_update()
    b.profile_reset(); b.profile_enable(1)
    assert b.region_extent_raw(r, 1, ok, masks, labels, constrain, 2, 3).shape == (1, 1, 6)
    launches = b.profile()['k_region_extent'][1]
    assert launches == 1
    bad = [((r, 1), ok + [[-1, 0, 0, 0]], 2, 2, None, 'anchor'), ((r, 1), ok + [[N, 0, 0, 0]], 2, 2, None, 'anchor'),
           ((r, 1), ok + [[3, len(MASKS), 0, 0]], 2, 2, None, 'mask index'), ((r, 1), ok + [[3, -2, 0, 0]], 2, 2, None, 'mask index'),
           ((r, 1), ok + [[3, 0, len(LABELS), 0]], 2, 2, None, 'label index'), ((r, 1), ok + [[3, 0, -2, 0]], 2, 2, None, 'label index'),
           ((r, 1), ok + [[3, 0, 0, 1]], 2, 2, None, 'fourth field'), ((r, 1), ok + [[3, 0, 0, -1]], 2, 2, None, 'fourth field'),
           ((r, 1), ok, -1, 2, None, 'window'), ((r, 1), ok, 2, -1, None, 'window'), ((r, 1), ok, 2048, 2048, None, 'window'),
           ((r, 1), ok, 2 ** 31 - 1, 2 ** 31 - 1, None, 'window'), ((r, 1), [], 2, 2, None, 'no queries'), ((r, 1), ok, 2, 2, 'masks', 'tables'),
           ((r, 1), ok, 2, 2, 'labels', 'tables'), ((r + 1, 1), ok, 2, 2, None, 'restart range'), ((-1, 1), ok, 2, 2, None, 'restart range'),
           ((r, 0), ok, 2, 2, None, 'restart range')]
    for (r0, nr), q, wl, wr, null, text in bad:
        assert _c_call(b, r0, nr, q, masks, labels, constrain, wl, wr, out, null) == bpmodel.RMX_EARG, (q, wl, wr, null, text)
        assert (out == -7.).all(), (q, wl, wr, null, text)                 # the output buffer is untouched
        assert re.search(text, hip._lib.load().rmx_last_error().decode()), (text, hip._lib.load().rmx_last_error())
        assert bpmodel.last_error_restarts() == []
        assert b.profile()['k_region_extent'][1] == launches, (q, wl, wr)   # nothing was launched
    assert _c_call(b, r, 1, ok, masks, labels, constrain, 2, 2, out, 'out') == bpmodel.RMX_EARG
    assert _c_call(b, r, 1, ok, masks, labels, constrain, 2047, 2048, np.zeros(4096)) == 0      # the widest window
    b.profile_enable(0)
    with pytest.raises(ValueError, match='^bad argument: .*mask index'):      # an index without a table
        b.region_extent_raw(r, 1, ok, None, labels, constrain, 2, 2)
    with pytest.raises(ValueError, match='^bad argument: .*window'):
        b.region_extent_raw(r, 1, ok, masks, labels, constrain, 4000, 4000)
    for kw in (dict(queries=[[0, 1, 0]]), dict(masks=masks[:, :, :-1]), dict(labels=labels[:1, :, :-1]), dict(constrain=np.ones(N + 1))):
        args = dict(queries=ok, masks=masks, labels=labels, constrain=None); args.update(kw)
        with pytest.raises(ValueError, match='must have shape'):
            b.region_extent_raw(r, 1, wl=2, wr=2, **args)
    for bad_call in (lambda: m.event_extent([30], 'loh'), lambda: m.event_extent([3], 'nothing'), lambda: m.event_extent([3], 'loh', -1),
                     lambda: m.event_extent([3], 'loh', 2048)):
        with pytest.raises(ValueError):
            bad_call()


def test_chunked_launch(hip, cases):
    """The widest window, 4 096 slots per query, and enough copies of three queries to need two launches."""
    case = cases[GRIDS[0]]
    b = case.b
    per = 4096
    reps = (64 << 20) // (per * 8 + 16) + 2
    few = _queries(case.anchors[:3], [('not_loh', 'total')])
    many = np.tile(few, ((reps + 2) // 3, 1))
    b.profile_reset(); b.profile_enable(1)
    big = b.region_extent_raw(case.r, 1, many, case.masks, case.labels, case.constrain, 2047, 2048)
    launches = b.profile()['k_region_extent'][1]; b.profile_enable(0)
    assert launches >= 2 and big.shape == (1, len(many), per)
    small = b.region_extent_raw(case.r, 1, few, case.masks, case.labels, case.constrain, 2047, 2048)
    assert np.array_equal(big[0].reshape(-1, 3, per), np.broadcast_to(small[0], (len(many) // 3, 3, per)))
    # the window covers every chain whole: the narrow window's slots, and -inf everywhere outside the chain
    narrow = _raw(case, case.anchors[:3], [('not_loh', 'total')])[0, :, 0]
    assert np.array_equal(small[0][:, 2047 - W:2047 + W + 1], narrow)
    for i, n0 in enumerate(case.anchors[:3]):
        c0, c1 = _chain(case, n0)
        n = n0 - 2047 + np.arange(per)
        assert np.isneginf(small[0, i][(n < c0) | (n > c1)]).all() and not np.isnan(small[0, i]).any() and np.isfinite(small[0, i, 2047])


def test_pipeline_cn_event_extents(hip, tmp_path):
    from remixt_amd import restarts, workflow
    from remixt_amd.analysis import pipeline
    from remixt_amd.restarts import RestartSet
    import pickle
    e, config, init_params = _pipeline_case()
    ids = sorted(init_params)
    seeds = [100 + i for i in ids]
    extents = [('del', 12, 'loh'), ('run', 77, 'state'), ('tot', 300, 'total'), ('both', 150, ('not_loh', 'total')), ('run2', 5, 'state')]
    names = [x[0] for x in extents]
    base = pipeline.fit_restarts(e, init_params, config, seeds=seeds, groups=1)
    off = pipeline.fit_restarts(e, init_params, dict(config, cn_event_extents=None, cn_extent_window=7), seeds=seeds, groups=1)
    on = pipeline.fit_restarts(e, init_params, dict(config, cn_event_extents=extents, cn_extent_window=20), seeds=seeds, groups=1)
    # unset: nothing of it in the results; set: the same results plus event_extents
    assert not any('event_extents' in res for res in base.values())
    _same_results(base, off)
    _same_results(base, dict((i, dict((k, v) for k, v in res.items() if k != 'event_extents')) for i, res in on.items()))
    # recomputation from the same fit
    rs = RestartSet(e, [init_params[i] for i in ids], 4, num_clones=3, quiet=True, seeds=seeds, **pipeline._model_kwargs(e, config))
    rs.fit(config['num_em_iter'], config['num_update_iter'])
    want = [rs.event_extent([seg], ev, 20) for _, seg, ev in extents]      # [entry][restart][0]
    rs.close()
    N = len(e.l)
    for j, i in enumerate(ids):
        ext = on[i]['event_extents']
        assert ext['names'] == names and sorted(ext) == sorted(posteriors.EXTENT_ARRAYS + ('names',))
        for a, (_, seg, _) in enumerate(extents):
            c = posteriors.compact_extents([want[a][j][0]])
            for k in posteriors.EXTENT_ARRAYS:
                assert ext[k].shape == (len(extents),) and ext[k][a] == c[k][0], (i, a, k)
            if ext['p_event'][a] > 0:
                assert 0 <= ext['left_q05'][a] <= ext['left_q50'][a] <= ext['left_q95'][a] <= seg <= ext['right_q05'][a] <= ext['right_q50'][a] <= ext['right_q95'][a] < N
                assert seg - ext['left_q05'][a] <= 20 and ext['right_q95'][a] - seg <= 20
        assert ((ext['p_event'] >= 0) & (ext['p_event'] <= 1)).all() and abs(ext['p_event'][1] - 1) <= 1e-12      # ('state' at one segment)
    one = pipeline.fit(e, init_params[ids[1]], dict(config, cn_event_extents=extents, cn_extent_window=20), quiet=True, init_id=ids[1])
    assert one['event_extents']['names'] == names and one['event_extents']['right_q50'].shape == (len(extents),)
    # the distributed form: the arrays through the record (its restarts run in two groups: compared with itself below)
    dist = restarts.fit_restarts_distributed(e, [init_params[i] for i in ids], 4, num_clones=3, num_em_iter=config['num_em_iter'],
                                             num_update_iter=config['num_update_iter'], seeds=seeds, quiet=True, cn_event_extents=extents,
                                             cn_extent_window=20, **pipeline._model_kwargs(e, config))
    for j, i in enumerate(ids):
        assert dist[j]['event_extents']['names'] == names
        for k in posteriors.EXTENT_ARRAYS:
            assert dist[j]['event_extents'][k].dtype == on[i]['event_extents'][k].dtype and dist[j]['event_extents'][k].shape == (len(extents),)
        assert np.abs(dist[j]['event_extents']['p_event'] - on[i]['event_extents']['p_event']).max() <= 1e-6
    # the workflow (fit_restarts_distributed + collate): the arrays in the store
    exp_file = str(tmp_path / 'experiment.pickle')
    with open(exp_file, 'wb') as f:
        pickle.dump(e, f)
    workflow.fit_model(exp_file, str(tmp_path / 'r.store'), dict(config, cn_event_extents=extents, cn_extent_window=20), None, seeds=seeds)
    with pipeline._Store(str(tmp_path / 'r.store'), 'r') as st:
        for i in sorted(st['stats']['init_id']):
            assert list(st['solutions/solution_%d/extent_names' % i]) == names
            for k in posteriors.EXTENT_ARRAYS:
                v = np.asarray(st['solutions/solution_%d/extent_%s' % (i, k)])
                assert np.array_equal(v, dist[ids.index(i)]['event_extents'][k]), (i, k)
    workflow.fit_model(exp_file, str(tmp_path / 'r0.store'), config, None, seeds=seeds)
    with pipeline._Store(str(tmp_path / 'r0.store'), 'r') as st:
        assert not any('extent_' in k for k in st.keys())


def test_against_the_sampler(hip):
    """4 096 sampled paths: the sampled boundary pmf within 4 binomial SDs of the exact one wherever the exact mass is above 1 %."""
    from tests.test_hip_posterior_summary import _fitted as fitted_masked
    m = fitted_masked(hip, 30, 3, 8, sweeps=3, masked=True)      # (read counts masked out: events of intermediate probability)
    case = Case(m)
    K = 4096
    st = case.b.sample_states(case.r, 1, K, [99]).astype(np.int64)[0]
    fwd, tel = np.asarray(m.seg_fwd_remap), np.asarray(m.is_telomere)
    rev = np.full(case.N, -1); rev[fwd] = np.arange(len(fwd))
    informative = 0
    for event in ('state', 'total', ('not_loh', None), ('not_subclonal', 'state')):
        mi, li = posteriors.parse_event(event)
        mk = None if mi < 0 else case.mask_seg[MASKS[mi]]
        lb = None if li < 0 else case.label_seg[LABELS[li]]
        anchors = list(range(1, len(fwd), 3))
        for a, s in zip(anchors, m.event_extent(anchors, event, W)):
            n0 = int(fwd[a])
            c0, c1 = _chain(case, n0)
            for side, step in (('right', 1), ('left', -1)):
                # per sample: how far the event holds from the anchor, in model segments
                alive = np.ones(K, dtype=bool)
                if mk is not None and case.constrain[n0]:
                    alive &= mk[n0, st[:, n0]]
                reach = np.where(alive, n0, -1)                      # the farthest model segment the event reaches; -1: not at the anchor
                n = n0
                while c0 <= n + step <= c1 and abs(n + step - n0) <= W:
                    if lb is not None:
                        alive &= lb[n, st[:, n]] == lb[n + step, st[:, n + step]]
                    n += step
                    if mk is not None and case.constrain[n]:
                        alive &= mk[n, st[:, n]]
                    reach = np.where(alive, n, reach)
                segs = s[side + '_segments']
                pmf = s[side + '_pmf']
                model_segs = fwd[segs]
                for i in range(len(pmf)):
                    # the boundary is segs[i]: the event reaches fwd[segs[i]] but not the next original segment
                    lo = model_segs[i]
                    if i + 1 < len(model_segs):
                        hit = (reach != -1) & ((reach - lo) * step >= 0) & ((reach - model_segs[i + 1]) * step < 0)
                    else:
                        hit = (reach != -1) & ((reach - lo) * step >= 0)
                    P = pmf[i]
                    if P > 0.01:
                        informative += P < 0.99
                        assert abs(hit.mean() - P) <= 4 * np.sqrt(P * (1 - min(P, 1.)) / K), (event, a, side, i, hit.mean(), P)
                if s[side + '_censored_mass'] > 0.01:
                    P = s[side + '_censored_mass']
                    hit = (reach != -1) & ((reach - model_segs[-1]) * step >= 0)
                    assert abs(hit.mean() - P) <= 4 * np.sqrt(P * (1 - min(P, 1.)) / K), (event, a, side, 'censored', hit.mean(), P)
    assert informative >= 3
