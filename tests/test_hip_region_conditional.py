"""Conditional posteriors given a region event on the device (rmx_region_conditional / k_region_conditional): against the numpy
twin (tests/conditional_twin.py) on the read-back framelogprob / log_transmat, the exact identities, bit identity across
restart ranges, query batches, groups, staging chunks and windows, two state classes, the mixed-model state, inserted
segments, no side effects on the model, every refusal, the public forms, and what the query is for."""
import ctypes as C
import re

import numpy as np
import pytest

from remixt_amd import posteriors, synthetic
from tests import conditional_twin
from tests import helpers as H
from tests.test_hip_region_events import CONSTRAINTS, LABELS, MASKS, Case
from tests.test_hip_sample_cn import GRIDS, _fitted, _model_state

pytestmark = pytest.mark.gpu

U = 2. ** -53
EPS = 1e-9      # per walked step, as the siblings hold log P


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


def _chain(case, n):
    c = int(np.searchsorted(case.ce, n, side='left'))
    return int(case.cs[c]), int(case.ce[c])


def _queries(runs, constraints):
    return np.array([[a, b, -1 if mk is None else MASKS.index(mk), -1 if lb is None else LABELS.index(lb)]
                     for (a, b) in runs for (mk, lb) in constraints], dtype=np.int32)


def _windows(case, q, window='chain'):
    if window == 'chain':
        return np.array([_chain(case, a) for a in q[:, 0]], dtype=np.int32)
    return np.array([(max(a - window, _chain(case, a)[0]), min(b + window, _chain(case, a)[1])) for a, b in q[:, :2]], dtype=np.int32)


def _over(err, bound):
    """err / bound per entry; where the bound is 0 (a weight column of zeros) the error has to be 0 too."""
    bound = np.broadcast_to(bound, np.shape(err))
    return np.where(bound > 0, err / np.where(bound > 0, bound, 1.), np.where(err == 0, 0., np.inf))


def _twin(case, a, b, lo, hi, mk, lb):
    """The twin's (cond, log P(E)) of a query, computed once per case."""
    cache = case.__dict__.setdefault('_cond_twin', {})
    key = (a, b, lo, hi, mk, lb)
    if key not in cache:
        cache[key] = conditional_twin.conditional(case.twin, a, b, lo, hi, None if mk is None else case.mask_seg[mk],
                                                  None if lb is None else case.label_seg[lb], case.constrain)
    return cache[key]


def _check(case, q, windows, logp, out, weights, states, tag):
    """One restart's rows against the twin, with the bounds of the issue: per entry Lw 1e-9 max|W[:, q]| on the projection, Lw 1e-9 on
    the maximum and the entry at the state, 2 Lw 1e-9 on the twin's value at the device's arg-max, L 1e-9 on P(E); -inf and
    NaN slots exactly where the twin's log P(E) is -inf; below -300 the comparison is printed, not asserted."""
    Q = weights.shape[2]
    wmax = np.abs(weights).max(axis=(0, 1))
    cls = case.b.seg_class
    worst, loud, impossible = 0., 0, 0
    for i, (a, b, mi, li) in enumerate(q.tolist()):
        lo, hi = int(windows[i, 0]), int(windows[i, 1])
        Lw, L = hi - lo + 1, b - a + 1
        mk, lb = (None if mi < 0 else MASKS[mi]), (None if li < 0 else LABELS[li])
        cond, lp = _twin(case, a, b, lo, hi, mk, lb)
        assert np.isnan(out[i, Lw:]).all(), (tag, i)                      # slots past hi
        rows = out[i, :Lw]
        if lp == -np.inf:
            impossible += 1
            assert logp[i] == -np.inf and np.isnan(rows).all(), (tag, a, b, mk, lb, logp[i])
            continue
        if lp < -300:
            loud += 1
            print('%s LOUD run [%d, %d] mask %s label %s: twin log P %.6g, device %.6g' % (tag, a, b, mk, lb, lp, logp[i]))
            continue
        assert abs(np.exp(logp[i]) - np.exp(lp)) <= L * EPS, (tag, a, b, mk, lb, logp[i], lp)
        assert not np.isnan(rows).any(), (tag, a, b, mk, lb)
        want = np.einsum('ks,ksq->kq', cond, weights[cls[lo:hi + 1]])
        e_proj = _over(np.abs(rows[:, :Q] - want), Lw * EPS * wmax).max()
        e_max = np.abs(rows[:, Q] - cond.max(axis=1)).max() / (Lw * EPS)
        am = rows[:, Q + 1].astype(int)
        assert (am == rows[:, Q + 1]).all() and (am >= 0).all() and (am < case.S).all()
        e_arg = (cond.max(axis=1) - cond[np.arange(Lw), am]).max() / (2 * Lw * EPS)
        e_st = 0. if states is None else np.abs(rows[:, Q + 2] - cond[np.arange(Lw), states[lo:hi + 1]]).max() / (Lw * EPS)
        if states is None:
            assert (rows[:, Q + 2] == 0).all()
        worst = max(worst, e_proj, e_max, e_arg, e_st)
        assert max(e_proj, e_max, e_arg, e_st) <= 1., (tag, a, b, mk, lb, e_proj, e_max, e_arg, e_st)
    print('%s: %d queries, %d impossible, %d below -300 (printed, not asserted), worst error / bound %.3e' % (tag, len(q), impossible, loud, worst))
    return worst


class CondCase(Case):
    def __init__(self, m, **kw):
        Case.__init__(self, m, **kw)
        self.weights, self.layout = posteriors.feature_matrix(self.b.cn_classes)
        self.amax = self.b.posterior_summary_raw(self.r, 1, want_stats=False)[2][0].astype(np.int16)      # a state per segment

    def cond(self, q, windows, weights=None, states='amax', r0=None, nr=1):
        st = self.amax if isinstance(states, str) else states
        if st is not None and nr > 1:
            st = np.broadcast_to(st, (nr, self.N))
        return self.b.region_conditional_raw(self.r if r0 is None else r0, nr, q, windows, self.masks, self.labels, self.constrain,
                                             self.weights if weights is None else weights, st)


@pytest.fixture(scope='module')
def cases(hip):
    return dict(((N, M, c), CondCase(_fitted(hip, N, M, c))) for N, M, c in GRIDS)


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_twin(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    assert case.S == {8: 165, 12: 355, 6: 457}[max_cn] and case.S % 64
    b = case.b
    q = _queries(case.queries(), CONSTRAINTS)
    windows = _windows(case, q)
    b.profile_reset(); b.profile_enable(1)
    logp, out = case.cond(q, windows)
    prof = b.profile(); b.profile_enable(0)
    assert prof['k_region_conditional'][1] == 1 and prof['k_region_conditional'][0] > 0
    nslot = int((windows[:, 1] - windows[:, 0] + 1).max())
    assert logp.shape == (1, len(q)) and out.shape == (1, len(q), nslot, case.layout['Q'] + 3)
    _check(case, q, windows, logp[0], out[0], case.weights, case.amax, 'S %d against the twin' % case.S)
    # without states the last entry is 0 and the rest is the same to the bit
    logp0, out0 = case.cond(q[:24], windows[:24], states=None)
    ns = out0.shape[2]                                                    # (the longest window of these queries)
    assert np.array_equal(logp0, logp[:, :24]) and np.array_equal(out0[..., :-1], out[:, :24, :ns, :-1], equal_nan=True)
    assert (out0[..., -1][~np.isnan(out0[..., 0])] == 0).all() and np.isnan(out[:, :24, ns:]).all()
    # the model-level form
    l1, o1 = case.m.model.region_conditional(q[:24], windows[:24], case.masks, case.labels, case.constrain, case.weights, case.amax)
    assert np.array_equal(l1, logp[0, :24]) and np.array_equal(o1, out[0, :24, :ns], equal_nan=True)


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_identities(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    b, S, Q = case.b, case.S, case.layout['Q']
    runs = case.queries()
    wmax = np.abs(case.weights).max(axis=(0, 1))
    proj, stats, amax = b.posterior_summary_raw(case.r, 1, weights=case.weights, states=case.amax[None])
    # without mask and label every slot is rmx_posterior_summary's, and log P(E) = 0
    q = _queries(runs, [(None, None)])
    windows = _windows(case, q)
    logp, out = case.cond(q, windows)
    for i, (a, e) in enumerate(runs):
        lo, hi = windows[i]
        Lw = hi - lo + 1
        rows = out[0, i, :Lw]
        assert abs(logp[0, i]) <= (e - a + 1) * (4 * S + 32) * U, (a, e, logp[0, i])
        assert (np.abs(rows[:, :Q] - proj[0, lo:hi + 1]) <= Lw * EPS * wmax).all(), (a, e)
        assert (np.abs(rows[:, Q] - stats[0, lo:hi + 1, 0]) <= Lw * EPS).all() and (np.abs(rows[:, Q + 2] - stats[0, lo:hi + 1, 2]) <= Lw * EPS).all()
        post = b.get_array(case.r, 'posterior_marginals')[lo:hi + 1]
        assert (post.max(axis=1) - post[np.arange(Lw), rows[:, Q + 1].astype(int)] <= 2 * Lw * EPS).all()
    print('S %d unconstrained: worst |proj - summary| / bound %.3e' % (S, max(
        _over(np.abs(out[0, i, :w[1] - w[0] + 1, :Q] - proj[0, w[0]:w[1] + 1]), (w[1] - w[0] + 1) * EPS * wmax).max() for i, w in enumerate(windows))))
    # inside a constrained run, a weight column that is the mask's complement gives exactly 0
    comp = np.ascontiguousarray(np.transpose(1. - case.masks, (0, 2, 1)))          # (C, S, masks)
    q = _queries(runs, [(k, None) for k in MASKS])
    windows = _windows(case, q)
    logp, out = case.cond(q, windows, weights=comp, states=None)
    checked = 0
    for i, (a, e, mi, _) in enumerate(q.tolist()):
        if np.isfinite(logp[0, i]):
            n = np.arange(a, e + 1)
            n = n[case.constrain[n]]
            col = out[0, i, n - windows[i, 0], mi]
            checked += len(col)
            assert (col == 0).all(), (a, e, MASKS[mi], col)
    assert checked > 0
    # log P(E) against rmx_region_prob on the same queries
    q = _queries(runs, CONSTRAINTS)
    windows = _windows(case, q, 2)
    logp, out2 = case.cond(q, windows)
    lp = b.region_logprob_raw(case.r, 1, q, case.masks, case.labels, case.constrain)
    assert np.array_equal(np.isneginf(logp), np.isneginf(lp))
    L = (q[:, 1] - q[:, 0] + 1)[None]
    assert (np.abs(np.exp(logp) - np.exp(lp)) <= L * EPS).all()
    # one-segment evidence, a mask and its complement: P(A) cond_A + P(not A) cond_notA is the unconditional projection
    mid = runs[0][0]
    assert runs[0] == (mid, mid) and case.constrain[mid]
    lo, hi = _chain(case, mid)
    for pair in (('loh', 'not_loh'), ('subclonal', 'not_subclonal')):
        q = _queries([(mid, mid)], [(k, None) for k in pair])
        logp, out = case.cond(q, _windows(case, q))
        mix = np.zeros((hi - lo + 1, Q))
        for j in range(2):
            if np.isfinite(logp[0, j]):
                mix += np.exp(logp[0, j]) * out[0, j, :hi - lo + 1, :Q]
        err = _over(np.abs(mix - proj[0, lo:hi + 1]), (hi - lo + 1) * EPS * wmax)
        print('S %d total probability over %s: P %s, worst error / bound %.3e' % (S, pair, np.exp(logp[0]), err.max()))
        assert (err <= 1.).all(), pair


@pytest.mark.parametrize('N,M,max_cn', GRIDS[:2])
def test_against_region_pattern(hip, cases, N, M, max_cn):
    """One feature F at three slots -- left of, inside and right of the run -- against P(E and F_n) / P(E) from rmx_region_pattern."""
    case = cases[(N, M, max_cn)]
    b = case.b
    c = int(np.argmax(case.ce - case.cs))
    seg = np.arange(case.cs[c], case.ce[c] + 1)
    real = seg[case.constrain[seg]]
    a = int(real[len(real) // 2 - 1])
    e = int(real[len(real) // 2])
    left, right = int(real[len(real) // 2 - 2]), int(real[len(real) // 2 + 1])
    ev, ft = MASKS.index('not_loh'), MASKS.index('not_subclonal')
    # a mask table with one more row: the evidence and the feature together, for the slot inside the run
    masks = np.concatenate([case.masks, (case.masks[:, ev] & case.masks[:, ft])[:, None]], axis=1)
    both = masks.shape[1] - 1
    feat = np.ascontiguousarray(np.transpose(case.masks[:, ft:ft + 1].astype(float), (0, 2, 1)))      # (C, S, 1): the feature's indicator
    q = np.array([[a, e, ev, -1]], dtype=np.int32)
    lo, hi = _chain(case, a)
    logp, out = b.region_conditional_raw(case.r, 1, q, [[lo, hi]], masks, case.labels, case.constrain, feat)
    assert np.isfinite(logp[0, 0])
    inner = [(a, a, both, -1), (e, e, ev, -1)] if a < e else [(a, a, both, -1)]
    pieces = np.array([(left, left, ft, -1), (a, e, ev, -1)] + inner + [(a, e, ev, -1), (right, right, ft, -1)], dtype=np.int32)
    pq = np.array([[0, 2, 0, 0], [2, len(inner), 0, 0], [2 + len(inner), 2, 0, 0]], dtype=np.int32)
    joint = b.region_pattern_raw(case.r, 1, pq, pieces, masks, case.labels, case.constrain)[0]
    for n, lj in zip((left, a, right), joint):
        want = np.exp(lj - logp[0, 0])
        got = out[0, 0, n - lo, 0]
        print('S %d segment %d: P(F | E) %.12g, pattern / evidence %.12g' % (case.S, n, got, want))
        assert abs(got - want) <= (hi - lo + 1) * EPS, (n, got, want)


def test_invariance(hip):
    """A (restart, query) slot is bit-identical alone, in a batch, in a restart range, across groups, in two staging chunks and
    under a narrower window that covers it."""
    from remixt_amd.restarts import RestartGroups, RestartSet
    e = synthetic.make_experiment(80, num_clones=3, max_copy_number=4, num_chains=3, seed=4)
    ps = synthetic.make_init_params(e, 4, 4)
    rs = RestartSet(e, ps, 4, num_clones=3, quiet=True, seeds=list(range(4)))
    rs.variational_update(2)
    b, m = rs.batch, rs.models[0]
    masks, labels = posteriors.event_tables(b.cn_classes)
    weights, layout = posteriors.feature_matrix(b.cn_classes)
    constrain = np.asarray(m.seg_is_original, dtype=np.uint8)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    chain = lambda n: (int(cs[np.searchsorted(ce, n)]), int(ce[np.searchsorted(ce, n)]))
    runs = [(n, min(n + k, chain(n)[1])) for n in range(0, b.num_segments, 7) for k in (0, 2)]
    q = np.array([[a, e_, mi, li] for (a, e_) in runs for mi, li in ((-1, -1), (1, -1), (-1, 1), (5, 2))], dtype=np.int32)
    wide = np.array([chain(a) for a in q[:, 0]], dtype=np.int32)
    call = lambda r0, nr, qq, ww: b.region_conditional_raw(r0, nr, qq, ww, masks, labels, constrain, weights)
    flogp, full = call(0, 4, q, wide)
    assert full.shape[:2] == (4, len(q)) and not np.array_equal(full[0], full[1], equal_nan=True) and np.isfinite(flogp).any()
    same = lambda x, y: np.array_equal(x, y, equal_nan=True)
    for r in range(4):
        lp, o = call(r, 1, q, wide)
        assert same(lp[0], flogp[r]) and same(o[0], full[r])
    lp, o = call(1, 2, q, wide)
    assert same(lp, flogp[1:3]) and same(o, full[1:3])
    for i in range(0, len(q), 5):
        lp, o = call(0, 4, q[i:i + 1], wide[i:i + 1])
        L = wide[i, 1] - wide[i, 0] + 1
        assert same(lp[:, 0], flogp[:, i]) and same(o[:, 0, :L], full[:, i, :L])
    lp, o = call(0, 4, q[::-1].copy(), wide[::-1].copy())
    assert same(lp, flogp[:, ::-1]) and same(o, full[:, ::-1])
    # narrower windows: the slots they keep
    for w in (0, 1, 5):
        narrow = np.stack([np.maximum(q[:, 0] - w, wide[:, 0]), np.minimum(q[:, 1] + w, wide[:, 1])], axis=1).astype(np.int32)
        lp, o = call(0, 4, q, narrow)
        assert same(lp, flogp)
        for i in range(len(q)):
            L = narrow[i, 1] - narrow[i, 0] + 1
            off = narrow[i, 0] - wide[i, 0]
            assert same(o[:, i, :L], full[:, i, off:off + L]), (w, i)
            assert np.isnan(o[:, i, L:]).all()
    # two staging chunks: 16 384 slots per query and one weight column leave room for 127 (restart, query) pairs in 64 MiB
    Q1 = np.ones((b.cn_classes.shape[0], b.num_cn_states, 1))
    few = q[:5]
    many = np.tile(few, (26, 1)); wmany = np.tile(wide[:5], (26, 1))
    small_lp, small = b.region_conditional_raw(0, 1, few, wide[:5], masks, labels, constrain, Q1)
    big_lp = np.zeros((1, len(many))); big = np.zeros((1, len(many), 16384, 4))
    b.profile_reset(); b.profile_enable(1)
    assert _c_call(b, 0, 1, many, wmany, 16384, masks, labels, constrain, Q1, None, big_lp, big) == 0
    launches = b.profile()['k_region_conditional'][1]; b.profile_enable(0)
    assert launches == 2, launches
    ns = small.shape[2]
    assert same(big_lp.reshape(26, 5), np.broadcast_to(small_lp, (26, 5))) and same(big[0, :, :ns].reshape(26, 5, ns, 4), np.broadcast_to(small[0], (26, 5, ns, 4)))
    assert np.isnan(big[0, :, ns:]).all()
    ok = np.isfinite(small[0, :, :, 0])
    assert ok.any() and (np.abs(small[0, :, :, 0][ok] - 1) <= 1e-12).all()          # a column of ones: the row sums
    # the public forms: one restart of a set, and groups against one group
    regions = [(0, 0), (11, 14), (40, 41), (20, 60)]
    per_set = rs.conditional_summary(regions, ('not_loh', 'total'))
    one = rs.models[2].conditional_summary(regions, ('not_loh', 'total'))
    assert len(per_set) == 4 and len(per_set[2]) == len(regions)
    for x, y in zip(per_set[2], one):
        assert sorted(x) == sorted(y) and all(same(x[k], y[k]) for k in x)
    rs.close()
    groups = RestartGroups(e, ps, 4, groups=2, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    single = RestartGroups(e, ps, 4, groups=1, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    for g in (groups, single):
        g.variational_update(2)
    x, y = groups.conditional_summary(regions, 'not_subclonal', 6), single.conditional_summary(regions, 'not_subclonal', 6)
    assert len(x) == len(y) == 4
    for r in range(4):
        for u, v in zip(x[r], y[r]):
            assert all(same(u[k], v[k]) for k in u)
    groups.close(); single.close()


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
        case = CondCase(m, batch=b, r=0)
        assert not np.array_equal(case.weights[0], case.weights[1])          # the weights differ per class
        q = _queries(case.queries()[:4], CONSTRAINTS)
        windows = _windows(case, q)
        logp, out = case.cond(q, windows)
        _check(case, q, windows, logp[0], out[0], case.weights, case.amax, 'two classes')
    finally:
        b.close()


def test_mixed_transition_model(hip):
    """The snapshot of the last update_p_cn under another transition_model than the current one, in both directions."""
    m = _fitted(hip, 40, 3, 4, seed=3)
    T0 = np.array(m.model.log_transmat)
    m.model.transition_model = 1
    assert np.array_equal(np.array(m.model.log_transmat), T0)            # the snapshot stays the model-0 one
    case = CondCase(m)
    q = _queries(case.queries()[:5], CONSTRAINTS)
    windows = _windows(case, q)
    logp, out = case.cond(q, windows)
    _check(case, q, windows, logp[0], out[0], case.weights, case.amax, 'mixed model 0 -> 1')
    m2 = _fitted(hip, 40, 3, 4, seed=3, transition_model=1)
    m2.model.transition_model = 0
    case2 = CondCase(m2)
    assert not np.array_equal(np.array(m2.model.log_transmat), T0)
    q = _queries(case2.queries()[:5], CONSTRAINTS[:1] + CONSTRAINTS[7:])
    windows = _windows(case2, q)
    logp, out = case2.cond(q, windows)
    _check(case2, q, windows, logp[0], out[0], case2.weights, case2.amax, 'mixed model 1 -> 0')


def test_inserted_segments(hip):
    """Two breakends on one boundary: the model inserts a zero-length segment there.  A mask does not bind it, the window counts
    it, and the public form drops it."""
    e = synthetic.make_experiment(60, num_clones=3, max_copy_number=4, num_chains=3, seed=7)
    e.breakpoints = H.add_shared_boundary_breakpoints(e)
    m, h, _ = H.make_model(hip, M=3, max_cn=4, experiment=e)
    H.attach(m, h)
    m.variational_update(); m.variational_update()
    case = CondCase(m)
    assert m.N1 > m.N and not case.constrain.all()
    dummy = int(np.flatnonzero(~case.constrain & (np.arange(m.N1) > 0) & (case.tel == 0))[0])
    q = _queries([(dummy - 1, dummy + 1), (dummy, dummy)], CONSTRAINTS)
    windows = _windows(case, q)
    logp, out = case.cond(q, windows)
    _check(case, q, windows, logp[0], out[0], case.weights, case.amax, 'inserted segment')
    # a mask alone on the inserted segment binds nothing: log P = 0 and the unconditional summary
    proj = case.b.posterior_summary_raw(case.r, 1, weights=case.weights, want_stats=False, want_argmax=False)[0][0]
    i = len(CONSTRAINTS) + CONSTRAINTS.index(('loh', None))
    lo, hi = windows[i]
    Q = case.layout['Q']
    assert abs(logp[0, i]) <= 1e-12 and (np.abs(out[0, i, :hi - lo + 1, :Q] - proj[lo:hi + 1]) <= (hi - lo + 1) * EPS * np.abs(case.weights).max(axis=(0, 1))).all()
    # the public form: experiment segments in, experiment order out
    fwd = np.asarray(m.seg_fwd_remap)
    k = int(np.flatnonzero(fwd == dummy - 1)[0])
    assert fwd[k + 1] == dummy + 1
    s = m.conditional_summary([(k, k + 1)], 'not_loh', 3)[0]
    qq = np.array([[dummy - 1, dummy + 1, MASKS.index('not_loh'), -1]], dtype=np.int32)
    ww = _windows(case, qq, 3)
    lp, o = case.cond(qq, ww, states=None)
    assert s['log_evidence'] == lp[0, 0] and s['p_loh'].shape == (m.N,) and 'cn_posterior_prob' not in s and 'cn_posterior_entropy' not in s
    inside = np.flatnonzero((fwd >= ww[0, 0]) & (fwd <= ww[0, 1]))
    assert np.array_equal(np.flatnonzero(~np.isnan(s['p_loh'])), inside) and len(inside) == ww[0, 1] - ww[0, 0]      # the inserted one is dropped
    assert np.array_equal(s['p_loh'][inside], o[0, 0, fwd[inside] - ww[0, 0], case.layout['loh']])
    assert (s['p_loh'][[k, k + 1]] == 0).all() and (s['cn_mpm'][inside] >= 0).all() and (np.delete(s['cn_mpm'], inside, axis=0) == -1).all()
    # with a decoded path: its probability given the event
    cn = np.zeros((m.N1, 3, 2), dtype=int)
    m.model.infer_cn(cn)
    s2 = m.conditional_summary([(k, k + 1)], 'not_loh', 3, cn=cn)[0]
    st = posteriors.cn_to_states(cn, case.b.cn_classes, case.b.seg_class)
    o2 = case.cond(qq, ww, states=st)[1]
    assert np.array_equal(s2['cn_posterior_prob'][inside], o2[0, 0, fwd[inside] - ww[0, 0], Q + 2])
    # against the unconditional summary
    sh = posteriors.evidence_shift(s, m.posterior_summary(), np.asarray(m.l1)[fwd])
    assert sh['log_evidence'] == s['log_evidence'] and np.isfinite(sh['ploidy_before']) and np.isfinite(sh['ploidy_after'])
    assert np.array_equal(~np.isnan(sh['p_loh']), ~np.isnan(s['p_loh'])) and (sh['p_loh'][[k, k + 1]] <= 0).all()


def test_no_side_effects(hip):
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    before = _model_state(m1)
    out = m1.conditional_summary([(0, 3), (20, 20), (40, 49)], ('not_loh', 'total'))
    assert len(out) == 3 and all(s['log_evidence'] <= 1e-12 for s in out)
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


def _c_call(b, r, nr, q, windows, nslot, masks, labels, constrain, weights, states, logp, out, null=None, Q=None):
    """rmx_region_conditional through ctypes with the caller's output buffers: the return code."""
    dp, ip, u8p, i16p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int16)
    q = np.ascontiguousarray(q, dtype=np.int32).reshape(-1, 4)
    windows = np.ascontiguousarray(windows, dtype=np.int32).reshape(-1, 2)
    masks, labels = np.ascontiguousarray(masks, dtype=np.uint8), np.ascontiguousarray(labels, dtype=np.int16)
    constrain = np.ascontiguousarray(constrain, dtype=np.uint8)
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    st = None if states is None else np.ascontiguousarray(states, dtype=np.int16)
    ptr = lambda arr, t, name: t() if null == name or arr is None or not arr.size else arr.ctypes.data_as(t)
    return b._lib.rmx_region_conditional(b._handle, r, nr, len(q), ptr(q, ip, 'queries'), ptr(windows, ip, 'windows'), nslot, masks.shape[1],
                                         ptr(masks, u8p, 'masks'), labels.shape[1], ptr(labels, i16p, 'labels'), constrain.ctypes.data_as(u8p),
                                         weights.shape[2] if Q is None else Q, ptr(weights, dp, 'weights'), ptr(st, i16p, 'states'),
                                         ptr(logp, dp, 'logp'), ptr(out, dp, 'out'))


def test_errors(hip):
    from remixt_amd import bpmodel
    m, h, e = H.make_model(hip, N=30, M=3, max_cn=3)
    H.attach(m, h)
    b, r = m.model._batch, m.model._r
    masks, labels = posteriors.event_tables(b.cn_classes)
    weights, layout = posteriors.feature_matrix(b.cn_classes)
    N, S, Q = b.num_segments, b.num_cn_states, layout['Q']
    constrain = np.ones(N, dtype=np.uint8)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    c = int(np.argmax(ce - cs))
    a0, end = int(cs[c]), int(ce[c])                                         # the longest chain
    assert end - a0 >= 5 and len(ce) > 1
    ok_q, ok_w, nslot = [[a0 + 2, a0 + 3, 0, 0]], [[a0, a0 + 5]], 8
    # a window, and a run, over a chain end next to it
    over_w = [[a0, end + 1]] if end + 1 < N else [[a0 - 1, a0 + 5]]
    over_q = [[end, end + 1, 0, 0]] if end + 1 < N else [[a0 - 1, a0, 0, 0]]
    logp, out = np.full(4, -7.), np.full(4 * nslot * (Q + 3), -7.)
    untouched = lambda: (logp == -7.).all() and (out == -7.).all()
    call = lambda q=ok_q, w=ok_w, ns=nslot, r0=r, nr=1, wt=weights, st=None, **kw: _c_call(b, r0, nr, q, w, ns, masks, labels, constrain, wt, st, logp, out, **kw)
    # before update_p_cn: RMX_EVALUE with the restart listed
    assert call() == bpmodel.RMX_EVALUE and untouched()
    with pytest.raises(ValueError, match='update_p_cn'):
        b.region_conditional_raw(r, 1, ok_q, ok_w, masks, labels, constrain, weights)
    assert bpmodel.last_error_restarts() == [r]
    with pytest.raises(ValueError, match='update_p_cn'):
        m.conditional_summary([(2, 3)], 'not_loh')
    m.variational_update()
    b.profile_reset(); b.profile_enable(1)
    assert call() == 0 and not untouched()
    logp[:] = -7.; out[:] = -7.
    launches = b.profile()['k_region_conditional'][1]
    assert launches == 1
    states = np.zeros((1, N), dtype=np.int16)
    bad_state = [states.copy(), states.copy()]
    bad_state[0][0, N - 1] = S; bad_state[1][0, 0] = -1
    bad = [(dict(q=ok_q + [[-1, 3, 0, 0]], w=ok_w * 2), 'first <= last'), (dict(q=ok_q + [[a0 + 4, a0 + 3, 0, 0]], w=ok_w * 2), 'first <= last'),
           (dict(q=[[N - 1, N, 0, 0]], w=[[N - 1, N]]), 'first <= last'),
           (dict(w=[[a0 + 3, a0 + 5]]), 'lo <= first'), (dict(w=[[a0, a0 + 2]]), 'lo <= first'), (dict(w=[[-1, a0 + 5]]), 'lo <= first'),
           (dict(w=[[a0, N]]), 'lo <= first'), (dict(w=over_w), 'chain end'), (dict(q=over_q, w=[over_q[0][:2]]), 'chain end'),
           (dict(ns=5), 'longer than nslot'), (dict(ns=0), 'nslot must be'), (dict(ns=16385), 'nslot must be'), (dict(ns=-1), 'nslot must be'),
           (dict(q=[[a0 + 2, a0 + 3, len(MASKS), 0]]), 'mask index'), (dict(q=[[a0 + 2, a0 + 3, -2, 0]]), 'mask index'),
           (dict(q=[[a0 + 2, a0 + 3, 0, len(LABELS)]]), 'label index'), (dict(q=[[a0 + 2, a0 + 3, 0, -2]]), 'label index'),
           (dict(Q=0), 'Q must be'), (dict(Q=65), 'Q must be'), (dict(Q=-1), 'Q must be'), (dict(null='weights'), 'Q must be'),
           (dict(st=bad_state[0]), 'state index'), (dict(st=bad_state[1]), 'state index'),
           (dict(q=[], w=[]), 'no queries'), (dict(null='windows'), 'no windows'), (dict(null='logp'), 'no windows'), (dict(null='out'), 'no queries'),
           (dict(null='masks'), 'tables'), (dict(null='labels'), 'tables'),
           (dict(r0=r + 1), 'restart range'), (dict(r0=-1), 'restart range'), (dict(nr=0), 'restart range')]
    for kw, text in bad:
        assert call(**kw) == bpmodel.RMX_EARG, (kw, text)
        assert untouched(), (kw, text)                                       # the output buffers are untouched
        assert re.search(text, hip._lib.load().rmx_last_error().decode()), (text, hip._lib.load().rmx_last_error())
        assert bpmodel.last_error_restarts() == []
        assert b.profile()['k_region_conditional'][1] == launches, kw        # nothing was launched
    # the evidence run's cap needs a model that long: rmxh::check_conditional's own test covers it (tests/test_conditional_host_cpu.py)
    assert call(st=states) == 0
    b.profile_enable(0)
    lib = hip._lib.load()
    ids = [i for i in range(lib.rmx_num_profile_ids()) if lib.rmx_profile_name(i) == b'k_region_conditional']
    assert len(ids) == 1 and ids[0] >= lib.rmx_num_kernels()
    ms, n = C.c_double(0.), C.c_int64(0)
    assert lib.rmx_profile_get(b._handle, ids[0], C.byref(ms), C.byref(n)) == 0 and n.value == launches + 1 and ms.value > 0
    assert lib.rmx_profile_get(b._handle, lib.rmx_num_profile_ids(), C.byref(ms), C.byref(n)) == bpmodel.RMX_EARG
    b.profile_reset()
    assert lib.rmx_profile_get(b._handle, ids[0], C.byref(ms), C.byref(n)) == 0 and n.value == 0 and 'k_region_conditional' not in b.profile()
    # the python forms
    with pytest.raises(ValueError, match='^bad argument: .*mask index'):      # an index without a table
        b.region_conditional_raw(r, 1, ok_q, ok_w, None, labels, constrain, weights)
    with pytest.raises(ValueError, match='^bad argument: .*Q must be'):
        b.region_conditional_raw(r, 1, ok_q, ok_w, masks, labels, constrain, np.ones((S, 65)))
    for kw in (dict(queries=[[0, 1, 0]]), dict(windows=[[0, 5], [0, 5]]), dict(masks=masks[:, :, :-1]), dict(labels=labels[:1, :, :-1]),
               dict(constrain=np.ones(N + 1)), dict(weights=weights[:, :-1]), dict(states=np.zeros((2, N)))):
        args = dict(queries=ok_q, windows=ok_w, masks=masks, labels=labels, constrain=None, weights=weights); args.update(kw)
        with pytest.raises(ValueError, match='must have shape'):
            b.region_conditional_raw(r, 1, **args)
    for bad_call in (lambda: m.conditional_summary([(30, 30)], 'loh'), lambda: m.conditional_summary([(3, 3)], 'nothing'),
                     lambda: m.conditional_summary([(3, 3)], 'loh', -1), lambda: m.conditional_summary([(3, 3)], 'loh', 'arm'),
                     lambda: m.conditional_summary([(3, 3)], np.ones((1, S + 1), dtype=bool))):
        with pytest.raises(ValueError):
            bad_call()
    assert m.conditional_summary([], 'loh') == []


def test_what_follows(hip):
    """The point of it: evidence "homozygous deletion" on one segment of a fitted model.  The normal rows of the usual state
    tables hold (1, 1), where no state is a homozygous deletion; here a stretch of one chain has a state class without normal
    copies, and the read counts are masked out so that the event has a probability worth printing."""
    m, h, e = H.make_model(hip, N=40, M=3, max_cn=4, chains=3)
    M = 3
    classes, _ = m._state_tables(M)
    classes = np.repeat(classes[:1], 2, axis=0)
    classes[1, :, 0, :] = (0, 0)
    N = m.N1
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    c = int(np.argmax(ce - cs))
    assert ce[c] - cs[c] >= 6
    seg_class = np.zeros(N, dtype=np.int32)
    seg_class[cs[c] + 1:cs[c] + 6] = 1
    brk_states = m.create_brk_states(M, m.max_copy_number, m.max_copy_number_diff)
    b = hip.RemixtBatch(M, N, m.num_breakpoints, m.normal_contamination, classes, seg_class, brk_states, np.asarray(h, dtype=float)[None],
                        m.l1, m.x1[:, 2].copy(), m.x1[:, 0:2].copy(), m.is_telomere, m.breakpoint_idx, m.breakpoint_orient,
                        m.transition_log_prob, [m.divergence_weight])
    try:
        b.set_array(0, 'allele_likelihood_mask', np.zeros(N, dtype=np.int64))
        b.set_array(0, 'total_likelihood_mask', np.zeros(N, dtype=np.int64))
        b.variational_update(2)
        fwd = np.asarray(m.seg_fwd_remap)
        real = np.flatnonzero((fwd >= cs[c] + 1) & (fwd <= cs[c] + 5))
        k = int(real[len(real) // 2])                                          # an experiment segment inside the stretch
        before = posteriors.batch_summaries(b, 0, 1)[0]
        s = posteriors.batch_conditional_summary(b, 0, 1, [(k, k)], 'hdel', 'chain', fwd, m.seg_is_original, m.is_telomere)[0][0]
        inside = np.flatnonzero((fwd >= cs[c]) & (fwd <= ce[c]))
        print('evidence: hdel at experiment segment %d, log evidence %.6f' % (k, s['log_evidence']))
        for j in inside:
            print('  segment %3d  p_hdel %.6f -> %.6f' % (j, before['p_hdel'][fwd[j]], s['p_hdel'][j]))
        assert np.isfinite(s['log_evidence']) and s['log_evidence'] < 0
        # segments of other chains are unchanged: outside the window
        outside = np.setdiff1d(np.arange(len(fwd)), inside)
        assert len(outside) and np.isnan(s['p_hdel'][outside]).all() and np.isnan(s['total_cn_mean'][outside]).all() and not np.isnan(s['p_hdel'][inside]).any()
        Lw = int(ce[c] - cs[c] + 1)
        assert abs(s['p_hdel'][k] - 1) <= Lw * EPS, s['p_hdel'][k]
    finally:
        b.close()
