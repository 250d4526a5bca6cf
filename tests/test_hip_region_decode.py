"""Region decode on the device (rmx_region_decode / k_region_decode): against the log-domain numpy twin on the read-back
framelogprob / log_transmat, identities on the device alone, state classes, the mixed-model state, inserted segments,
invariance to batching, grouping, padding and chunking, no side effects on the model, errors, the public forms and the
pipeline.

Tolerance: the family's bound, L 1e-9 in log P for a run of L segments.  Paths are not compared with
the twin's path for equality -- rounding-level near-ties exist on real fits -- but through their own
probability: for every query with a finite result
  1. the returned path satisfies the event exactly, and entries past the run are -1;
  2. |logp_out - twin log-probability of the returned path| <= L 1e-9;
  3. twin log-probability of the returned path >= twin optimum - 2 L 1e-9 (a comparison perturbed by rounding can cost at
     most the bound on each side);
  4. -inf on the device exactly where the twin's optimum is -inf, the states then -1."""
import ctypes as C

import numpy as np
import pytest

from remixt_amd import posteriors, synthetic
from tests import call_twin, decode_twin
from tests import helpers as H
from tests.test_hip_region_events import LABELS, MASKS, Case
from tests.test_hip_region_pattern import _breakend, _longest
from tests.test_hip_region_span import CHAINS, CONSTRAINTS
from tests.test_hip_sample_cn import GRIDS, _fitted, _model_state, _pipeline_case, _same_results

pytestmark = pytest.mark.gpu

U = 2. ** -53
BOUND = 1e-9
OUT_BUDGET, BP_BUDGET = 64 << 20, 1 << 30      # (rmxh::DECODE_OUT_BUDGET, DECODE_BP_BUDGET)


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


def _queries(runs, constraints=CONSTRAINTS):
    return np.array([[a, b, -1 if mk is None else MASKS.index(mk), -1 if lb is None else LABELS.index(lb)]
                     for (a, b) in runs for (mk, lb) in constraints], dtype=np.int32)


def _raw(case, runs, constraints=CONSTRAINTS, r0=None, nr=1, max_len=None):
    logp, states = case.b.region_decode_raw(case.r if r0 is None else r0, nr, _queries(runs, constraints), case.masks, case.labels, case.constrain, max_len)
    return logp.reshape(nr, len(runs), len(constraints)), states.reshape(nr, len(runs), len(constraints), -1)


def _runs(case):
    """A 10-segment run, the whole longest chain, a run across a breakend adjacency, one-segment runs."""
    c0, c1 = _longest(case)
    be = _breakend(case)
    mid = (c0 + c1) // 2
    return [(c0, c0 + 9), (c0, c1), (be - 3, be + 4), (mid, mid), (c0, c0), (c1, c1), (be, be)]


def _tables(case, mk, lb):
    return (None if mk is None else case.mask_seg[mk]), (None if lb is None else case.label_seg[lb])


def _path_logprob(case, a, b, path):
    """Twin log-probability of the run's configuration `path`: every segment of the run binds, the inserted ones included."""
    full = np.zeros(case.N, dtype=np.int64)
    full[a:b + 1] = path
    return call_twin.logprob(case.twin, a, b, None, full)


def _check(case, runs, logp, states, want, tag, constraints=CONSTRAINTS):
    """The four checks of the module docstring for one restart's results; returns (finite results, all results)."""
    worst, finite = 0., 0
    for i, (a, b) in enumerate(runs):
        L = b - a + 1
        for j, (mk, lb) in enumerate(constraints):
            g, st, (w, _) = logp[i, j], states[i, j], want[i][j]
            assert not np.isnan(g), (tag, a, b, mk, lb)
            assert (g == -np.inf) == (w == -np.inf), (tag, a, b, mk, lb, g, w)
            assert (st[L:] == -1).all(), (tag, a, b, mk, lb)
            if g == -np.inf:
                assert (st == -1).all(), (tag, a, b, mk, lb)
                continue
            finite += 1
            mask, label = _tables(case, mk, lb)
            assert (st[:L] >= 0).all() and (st[:L] < case.S).all()
            assert decode_twin.satisfies(st[:L], a, b, mask, label, case.constrain), (tag, a, b, mk, lb, st[:L])
            own = _path_logprob(case, a, b, st[:L])
            e2, e3 = abs(g - own) / (L * BOUND), (w - own) / (2 * L * BOUND)
            worst = max(worst, e2, e3)
            print('%s run [%d, %d] mask %s label %s: log P* %.17g, its path by the twin %.17g, twin optimum %.17g' % (tag, a, b, mk, lb, g, own, w))
            assert e2 <= 1., (tag, a, b, mk, lb, g, own)
            assert e3 <= 1., (tag, a, b, mk, lb, own, w)
    print('%s: worst error / bound %.3e over %d finite results of %d' % (tag, worst, finite, len(runs) * len(constraints)))
    return finite, len(runs) * len(constraints)


def _want(case, runs, constraints=CONSTRAINTS):
    return [[decode_twin.decode(case.twin, a, b, *_tables(case, mk, lb), case.constrain) for mk, lb in constraints] for a, b in runs]


class DecodeCase(Case):
    def __init__(self, m, **kw):
        Case.__init__(self, m, **kw)
        self.runs = _runs(self)
        self.want = _want(self, self.runs)      # (computed once, shared by the tests of the grid)


@pytest.fixture(scope='module')
def cases(hip):
    return dict(((N, M, c), DecodeCase(_fitted(hip, N, M, c, chains=CHAINS[c]))) for N, M, c in GRIDS)


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_twin(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    assert case.S == {8: 165, 12: 355, 6: 457}[max_cn] and case.S % 64
    b = case.b
    b.profile_reset(); b.profile_enable(1)
    logp, states = _raw(case, case.runs)
    prof = b.profile(); b.profile_enable(0)
    assert prof['k_region_decode'][1] == 1 and prof['k_region_decode'][0] > 0
    assert states.shape[-1] == max(z - a + 1 for a, z in case.runs) and states.dtype == np.int16
    finite, total = _check(case, case.runs, logp[0], states[0], case.want, 'S %d' % case.S)
    assert 2 * finite >= total
    # the model-level form
    q = _queries(case.runs)
    one_p, one_s = case.m.model.region_decode(q, case.masks, case.labels, case.constrain)
    assert one_p.shape == (len(q),) and np.array_equal(one_p, logp[0].ravel()) and np.array_equal(one_s, states[0].reshape(len(q), -1))


def _call_states(case):
    path = np.zeros((case.m.model.num_segments, case.m.model.num_clones, case.m.model.num_alleles), dtype=int)
    case.m.model.infer_cn(path)
    return posteriors.cn_to_states(path, case.b.cn_classes, case.b.seg_class)


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_identities(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    b, S, r = case.b, case.S, case.r
    logp, states = _raw(case, case.runs)
    logp, states = logp[0], states[0]
    # a one-segment query: the state is numpy.argmax of the masked read-back marginals, exactly; the value is their maximum
    post = b.get_array(r, 'posterior_marginals')
    ns = np.arange(case.N)
    for j, k in enumerate((None,) + tuple(MASKS)):
        q = np.array([[n, n, -1 if k is None else MASKS.index(k), -1] for n in ns], dtype=np.int32)
        lp, st = b.region_decode_raw(r, 1, q, case.masks, case.labels, case.constrain)
        row = post if k is None else np.where(case.mask_seg[k] | ~case.constrain[:, None], post, 0.)
        want = row.max(axis=1)
        assert st.shape == (1, case.N, 1)
        assert np.array_equal(lp[0] == -np.inf, want == 0) and np.array_equal(st[0, :, 0], np.where(want > 0, np.argmax(row, axis=1), -1)), k
        ok = want > 0
        tol = ((S + 4) + 3 * np.abs(np.log(want[ok]))) * U
        assert (np.abs(np.exp(lp[0, ok]) / want[ok] - 1) <= tol).all(), k
    # the value is the log-probability of the returned path (rmx_call_prob, label -1, every segment binds); the maximum is not
    # above the sum (rmx_region_prob)
    q = _queries(case.runs)
    Lq = (q[:, 1] - q[:, 0] + 1).astype(float)
    flat_p, flat_s = logp.ravel(), states.reshape(len(q), -1)
    fin = np.isfinite(flat_p)
    paths = np.zeros((1, len(q), case.N), dtype=np.int16)
    for i in np.flatnonzero(fin):
        paths[0, i, q[i, 0]:q[i, 1] + 1] = flat_s[i, :int(Lq[i])]
    qc = np.stack([q[:, 0], q[:, 1], np.full(len(q), -1), np.arange(len(q))], axis=1).astype(np.int32)
    own = b.call_logprob_raw(r, 1, paths, qc, case.labels, None)[0]
    assert (np.abs(flat_p[fin] - own[fin]) <= 2 * Lq[fin] * BOUND).all(), np.abs(flat_p[fin] - own[fin]).max()
    total = b.region_logprob_raw(r, 1, q, case.masks, case.labels, case.constrain)[0]
    assert np.array_equal(total == -np.inf, ~fin) and (flat_p[fin] <= total[fin] + Lq[fin] * BOUND).all()
    print('S %d: max |log P* - call_logprob of its path| %.3e, min log P(E) - log P* %.3e' % (S, np.abs(flat_p[fin] - own[fin]).max(), (total[fin] - flat_p[fin]).min()))
    # a mask that admits one state per class forces a constant path: maximum and sum are then the same single term
    call = _call_states(case)
    c0, c1 = _longest(case)
    s0 = int(np.bincount(call[c0:c0 + 10], minlength=S).argmax())
    one = np.zeros((b.cn_classes.shape[0], 1, S), dtype=np.uint8); one[:, 0, s0] = 1
    q1 = np.array([[c0, c0 + 9, 0, -1], [c0 + 2, c0 + 2, 0, -1]], dtype=np.int32)
    lp1, st1 = b.region_decode_raw(r, 1, q1, one, None, None)
    sum1 = b.region_logprob_raw(r, 1, q1, one, None, None)[0]
    assert np.isfinite(lp1[0]).all() and (st1[0, 0] == s0).all() and st1[0, 1, 0] == s0 and (st1[0, 1, 1:] == -1).all()
    assert (np.abs(lp1[0] - sum1) <= np.array([10, 1]) * BOUND).all(), (lp1, sum1)
    # the whole chain without a constraint against the genome-wide decode: both maximise q of the chain's path
    whole = np.array([[int(a), int(z), -1, -1] for a, z in zip(case.cs, case.ce)], dtype=np.int32)
    lpw, stw = b.region_decode_raw(r, 1, whole, None, None, None)
    vit = b.call_logprob_raw(r, 1, call[None, None].astype(np.int16), np.array([[a, z, -1, 0] for a, z, _, _ in whole], dtype=np.int32), None, None)[0]
    Lw = (whole[:, 1] - whole[:, 0] + 1).astype(float)
    print('S %d whole chains: log P* %s, log q of the decoded path %s' % (S, lpw[0], vit))
    assert (np.abs(lpw[0] - vit) <= 2 * Lw * BOUND).all()
    # no sampled path that satisfies the event is more probable than the maximum
    K = 256
    smp = b.sample_states(r, 1, K, [11])                                   # (1, K, N)
    assert smp.shape == (1, K, case.N)
    sel = [i for i in range(len(q)) if fin[i] and Lq[i] > 1]
    qs = np.array([[q[i, 0], q[i, 1], -1, k] for i in sel for k in range(K)], dtype=np.int32)
    lps = b.call_logprob_raw(r, 1, smp.astype(np.int16), qs, None, None)[0].reshape(len(sel), K)
    hits = 0
    for row, i in enumerate(sel):
        a, z = int(q[i, 0]), int(q[i, 1])
        mk, lb = CONSTRAINTS[i % len(CONSTRAINTS)]
        mask, label = _tables(case, mk, lb)
        for k in range(K):
            if decode_twin.satisfies(smp[0, k, a:z + 1], a, z, mask, label, case.constrain):
                hits += 1
                assert lps[row, k] <= flat_p[i] + 2 * Lq[i] * BOUND, (a, z, mk, lb, k, lps[row, k], flat_p[i])
    assert hits > 0
    print('S %d: %d sampled sub-paths satisfy their event, none above log P*' % (S, hits))


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
        runs = _runs(case)[:4]
        logp, states = _raw(case, runs)
        _check(case, runs, logp[0], states[0], _want(case, runs), 'two classes')
        # LOH is possible only at the odd segments: a run of two is impossible, an odd segment alone is not
        odd = [n for n in range(3, N - 2, 2) if case.tel[n - 1] == 0 and case.tel[n] == 0]
        lp, st = _raw(case, [(n, n) for n in odd] + [(n, n + 1) for n in odd], [('loh', None)])
        assert np.isfinite(lp[0, :len(odd), 0]).all() and np.isneginf(lp[0, len(odd):, 0]).all() and (st[0, len(odd):] == -1).all()
        assert all(loh[1][s] for s in st[0, :len(odd), 0, 0])
    finally:
        b.close()


def test_mixed_transition_model(hip):
    """Restarts 0 and 3 keep their model-0 snapshot, restarts 1 and 2 take theirs under model 1: a call over 0 .. 3 has three
    runs of restarts and equals the single-restart calls bit for bit; restarts 0 and 1 agree with the twin on their own
    snapshot (exp(trans_value) on plain adjacencies too for restart 0)."""
    from tests.test_hip_query_driver import _restart_set
    rs = _restart_set(4)
    try:
        b = rs.batch
        b.transition_model = 1
        b.update_p_cn(1, 3)
        cases = [Case(rs.models[r]) for r in (0, 1)]
        case = cases[0]
        c = int(np.argmax(case.ce - case.cs))
        c0, c1 = int(case.cs[c]), int(case.ce[c])
        runs = [(c0, c1), (c0 + 1, min(c0 + 8, c1)), (c0 + 2, c0 + 2), (int(case.cs[1]), int(case.cs[1]) + 1)]
        q = _queries(runs)
        call = lambda r0, nr: b.region_decode_raw(r0, nr, q, case.masks, case.labels, case.constrain)
        b.profile_reset(); b.profile_enable(1)
        full_p, full_s = call(0, 4)
        launches = b.profile()['k_region_decode'][1]; b.profile_enable(0)
        assert launches == 3
        assert len(np.unique(full_p, axis=0)) > 1
        for r in range(4):
            p, s = call(r, 1)
            assert np.array_equal(p[0], full_p[r]) and np.array_equal(s[0], full_s[r]), r
        p, s = call(1, 3)
        assert np.array_equal(p, full_p[1:]) and np.array_equal(s, full_s[1:])
        for cs_ in cases:
            shape = (len(runs), len(CONSTRAINTS))
            _check(cs_, runs, full_p[cs_.r].reshape(shape), full_s[cs_.r].reshape(shape + (-1,)), _want(cs_, runs), 'mixed model, restart %d' % cs_.r)
    finally:
        rs.close()


def _inserted_model(hip):
    e = synthetic.make_experiment(60, num_clones=3, max_copy_number=4, num_chains=3, seed=7)
    e.breakpoints = H.add_shared_boundary_breakpoints(e)
    m, h, _ = H.make_model(hip, M=3, max_cn=4, experiment=e)
    H.attach(m, h)
    m.model.allele_likelihood_mask = np.zeros(m.model.num_segments, dtype=int)      # (events of intermediate probability)
    m.variational_update(); m.variational_update()
    return m


def _twin_batch(case):
    return decode_twin.DecodeTwinBatch(case.b.cn_classes, case.b.seg_class, [case.b.get_array(case.r, 'framelogprob')],
                                       [case.b.get_array(case.r, 'log_transmat')], case.cs, case.ce)


def _check_region_call(got, want, regions, m, case, call_states, event, tag):
    """region_call's dict of one restart against batch_region_calls over the twin (restart 0 of `want`)."""
    cs, ce = case.cs, case.ce
    runs, piece_region, _ = posteriors.region_queries(np.array([r[-2:] for r in regions]), m.seg_fwd_remap, m.seg_is_original, cs, ce)
    fwd = np.asarray(m.seg_fwd_remap)
    for k in range(len(regions)):
        Lk = float(sum(z - a + 1 for (a, z), p in zip(runs, piece_region) if p == k))
        for key in ('log_prob', 'log_p_event', 'log_prob_call'):
            g, w = got[key][k], want[key][0, k]
            print('%s region %s %s: %.17g (twin %.17g)' % (tag, regions[k], key, g, w))
            assert (g == -np.inf and w == -np.inf) or abs(g - w) <= 2 * Lk * BOUND, (tag, k, key, g, w)
        if np.isfinite(got['log_prob'][k]):
            assert got['log_prob_given_event'][k] <= 0 and abs(got['log_prob_given_event'][k] - (got['log_prob'][k] - got['log_p_event'][k])) <= 1e-12
            seg = fwd[regions[k][-2]:regions[k][-1] + 1]
            assert got['cn'][k].shape == (len(seg), 3, 2)
            own = np.array([int(np.flatnonzero((case.b.cn_classes[case.b.seg_class[n]] == got['cn'][k][i]).all(axis=(1, 2)))[0]) for i, n in enumerate(seg)])
            assert got['n_differ'][k] == (own != call_states[seg]).sum()
            if event is not None and event[0] is not None:
                assert all(case.mask_seg[event[0]][n, s] for n, s in zip(seg, own))


def test_inserted_segments(hip):
    """Two breakends on one boundary: the model inserts a zero-length segment there.  A mask does not bind it, a label binds
    the adjacencies through it, its state is part of the configuration, and region_call reports the original segments."""
    m = _inserted_model(hip)
    case = Case(m)
    assert m.N1 > m.N and not case.constrain.all()
    dummy = int(np.flatnonzero(~case.constrain & (np.arange(m.N1) > 0) & (case.tel == 0))[0])
    runs = [(dummy - 1, dummy + 1), (dummy, dummy), (dummy, dummy + 1), (dummy - 3, dummy + 2)]
    logp, states = _raw(case, runs)
    _check(case, runs, logp[0], states[0], _want(case, runs), 'inserted segment')
    lp, _ = _raw(case, [(dummy, dummy)], [(k, None) for k in MASKS])
    assert np.isfinite(lp).all() and len(np.unique(lp)) == 1                 # no mask binds the inserted segment, 'hdel' included
    i = int(m.seg_rev_remap[dummy - 1])
    fwd = np.asarray(m.seg_fwd_remap)
    assert fwd[i] == dummy - 1 and fwd[i + 1] == dummy + 1
    regions = [(i, i + 1), (i - 2, i), (i + 1, i + 1), (0, 2), (m.N - 2, m.N - 1), (0, m.N - 1)]
    tb = _twin_batch(case)
    call = _call_states(case)
    for event in (None, ('not_subclonal', None), (None, 'total'), ('not_loh', 'total')):
        got = m.region_call(regions, event)
        want = posteriors.batch_region_calls(tb, 0, 1, regions, m.seg_fwd_remap, m.seg_is_original, m.is_telomere, event=event, cn=call[None])
        _check_region_call(got, want, regions, m, case, call, event, 'event %s' % (event,))
    # the whole genome without an event: the regional configuration of every chain is as probable as the decoded path
    got = m.region_call([(0, m.N - 1)])
    assert got['cn'][0].shape == (m.N, 3, 2) and got['log_prob'][0] <= 0


def test_invariance(hip):
    """A (restart, query) result, value and path, is bit-identical in any restart range, any batch and order of queries, for
    any max_len, across RestartSet / RestartGroups, and in a call that runs in several chunks."""
    from remixt_amd.restarts import RestartGroups, RestartSet
    e = synthetic.make_experiment(80, num_clones=3, max_copy_number=4, num_chains=3, seed=4)
    ps = synthetic.make_init_params(e, 4, 4)
    rs = RestartSet(e, ps, 4, num_clones=3, quiet=True, seeds=list(range(4)))
    rs.variational_update(2)
    b, m = rs.batch, rs.models[0]
    S = b.num_cn_states
    masks, labels = posteriors.event_tables(b.cn_classes)
    constrain = np.asarray(m.seg_is_original, dtype=np.uint8)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    runs = []
    for c0, c1 in zip(cs, ce):
        c0, c1 = int(c0), int(c1)
        assert c1 - c0 >= 14
        runs += [(c0, c1), (c0 + 1, c0 + 9), (c0 + 3, c0 + 3), (c1 - 4, c1)]
    q = _queries(runs)
    longest = int((q[:, 1] - q[:, 0] + 1).max())
    call = lambda r0, nr, qq, ml=None: b.region_decode_raw(r0, nr, qq, masks, labels, constrain, ml)
    full_p, full_s = call(0, 4, q)
    assert full_p.shape == (4, len(q)) and full_s.shape == (4, len(q), longest) and not np.isnan(full_p).any()
    assert not np.array_equal(full_p[0], full_p[1]) and 2 * np.isfinite(full_p).sum() >= full_p.size
    for r in range(4):
        p, s = call(r, 1, q)
        assert np.array_equal(p[0], full_p[r]) and np.array_equal(s[0], full_s[r])
    p, s = call(1, 2, q)
    assert np.array_equal(p, full_p[1:3]) and np.array_equal(s, full_s[1:3])
    # single queries (max_len: that query's own length), and the queries in another order
    for i in range(0, len(q), 5):
        p, s = call(0, 4, q[i:i + 1])
        L = int(q[i, 1] - q[i, 0] + 1)
        assert s.shape[2] == L and np.array_equal(p[:, 0], full_p[:, i]) and np.array_equal(s[:, 0], full_s[:, i, :L])
    p, s = call(0, 4, q[::-1].copy())
    assert np.array_equal(p, full_p[:, ::-1]) and np.array_equal(s, full_s[:, ::-1])
    # padding: max_len 4096 against the longest query
    p, s = call(0, 4, q, 4096)
    assert s.shape == (4, len(q), 4096) and np.array_equal(p, full_p) and np.array_equal(s[:, :, :longest], full_s) and (s[:, :, longest:] == -1).all()
    # several chunks: at max_len 4096 a strip is 4096 S int16, and rmxh::decode_plan gives chunks of `qc` queries for 4 restarts
    strips = BP_BUDGET // (4096 * S * 2)
    qc = min(strips // 4, (OUT_BUDGET - 8) // (4 * (8 + 2 * 4096) + 16))
    reps = qc // len(q) + 1
    many = np.tile(q, (reps, 1))
    assert qc < len(many) < 4 * qc
    b.profile_reset(); b.profile_enable(1)
    p, s = call(0, 4, many, 4096)
    ms, launches = b.profile()['k_region_decode']; b.profile_enable(0)
    print('k_region_decode: 4 restarts x %d queries at max_len 4096, %d states, chunks of %d: %.2f ms device in %d launches' % (len(many), S, qc, ms, launches))
    assert launches >= 2 and launches == -(-len(many) // qc)
    assert np.array_equal(p.reshape(4, reps, len(q)), np.broadcast_to(full_p[:, None], (4, reps, len(q))))
    assert np.array_equal(s.reshape(4, reps, len(q), 4096)[..., :longest], np.broadcast_to(full_s[:, None], (4, reps, len(q), longest)))
    assert (s[..., longest:] == -1).all()
    # the public forms: one restart of a set, and groups against one group
    regions = [(4, 12), (20, 20), (0, 1), (30, 60)]
    for event in (None, ('not_loh', 'total')):
        per_set, one = rs.region_call(regions, event), rs.models[2].region_call(regions, event)
        for k in ('log_prob', 'log_p_event', 'log_prob_given_event', 'n_differ', 'log_prob_call'):
            assert per_set[k].shape == (4, len(regions)) and np.array_equal(per_set[k][2], one[k], equal_nan=True), k
        assert all(np.array_equal(x, y) for x, y in zip(per_set['cn'][2], one['cn']))
    rs.close()
    groups = RestartGroups(e, ps, 4, groups=2, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    single = RestartGroups(e, ps, 4, groups=1, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    for g in (groups, single):
        g.variational_update(2)
    x, y = groups.region_call(regions, ('not_loh', 'total')), single.region_call(regions, ('not_loh', 'total'))
    for k in ('log_prob', 'log_p_event', 'log_prob_given_event', 'n_differ', 'log_prob_call'):
        assert x[k].shape == (4, len(regions)) and np.array_equal(x[k], y[k], equal_nan=True), k
    assert len(x['cn']) == 4 and all(np.array_equal(u, v) for xr, yr in zip(x['cn'], y['cn']) for u, v in zip(xr, yr))
    groups.close(); single.close()


def test_no_side_effects(hip):
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    before = _model_state(m1)
    out = m1.region_call([(0, 9), (20, 22), (40, 49)], ('not_loh', 'state'))
    assert (out['log_prob'] <= 0).all()
    out = m1.region_call([(0, 49)])
    assert np.isfinite(out['log_prob']).all() and out['n_differ'][0] >= 0
    after = _model_state(m1)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    # a fit continued after the calls equals one without them
    for m in (m1, m2):
        m.variational_update()
        m.variational_update()
    s1, s2 = _model_state(m1), _model_state(m2)
    for k in s1:
        assert np.array_equal(s1[k], s2[k], equal_nan=True), k
    assert m1.model.calculate_elbo() == m2.model.calculate_elbo()


def _c_call(b, r, nr, q, masks, labels, constrain, max_len, states, out, null=None, nq=None):
    """rmx_region_decode through ctypes with the caller's output buffers: the return code."""
    dp, ip, u8p, i16p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int16)
    q = np.ascontiguousarray(q, dtype=np.int32).reshape(-1, 4)
    masks, labels = np.ascontiguousarray(masks, dtype=np.uint8), np.ascontiguousarray(labels, dtype=np.int16)
    constrain = np.ascontiguousarray(constrain, dtype=np.uint8)
    return b._lib.rmx_region_decode(b._handle, r, nr, len(q) if nq is None else nq, q.ctypes.data_as(ip) if len(q) else ip(),
                                    masks.shape[1], u8p() if null == 'masks' else masks.ctypes.data_as(u8p), labels.shape[1],
                                    i16p() if null == 'labels' else labels.ctypes.data_as(i16p), constrain.ctypes.data_as(u8p), max_len,
                                    i16p() if null == 'states' else states.ctypes.data_as(i16p), dp() if null == 'out' else out.ctypes.data_as(dp))


def test_errors(hip):
    import re
    from remixt_amd import bpmodel
    m, h, e = H.make_model(hip, N=30, M=3, max_cn=3)
    H.attach(m, h)
    b, r = m.model._batch, m.model._r
    masks, labels = posteriors.event_tables(b.cn_classes)
    N = b.num_segments
    constrain = np.ones(N, dtype=np.uint8)
    cs, ce = posteriors.chains_from_telomeres(np.asarray(m.is_telomere))
    e0, s1 = int(ce[0]), int(cs[1])
    assert e0 >= 6 and len(cs) >= 2
    okq = [[0, 2, 0, 0], [4, 4, -1, -1]]
    out, states = np.full(8, -7.), np.full(64, -9, dtype=np.int16)
    untouched = lambda: (out == -7.).all() and (states == -9).all()
    # before update_p_cn: RMX_EVALUE with the restart listed
    assert _c_call(b, r, 1, okq, masks, labels, constrain, 3, states, out) == bpmodel.RMX_EVALUE and untouched()
    with pytest.raises(ValueError, match='update_p_cn'):
        b.region_decode_raw(r, 1, okq, masks, labels, constrain)
    assert bpmodel.last_error_restarts() == [r]
    with pytest.raises(ValueError, match='update_p_cn'):
        m.region_call([(0, 1)], None, np.ones((m.N, 3, 2), dtype=int))
    m.variational_update()
    b.profile_reset(); b.profile_enable(1)
    p, s = b.region_decode_raw(r, 1, okq, masks, labels, constrain)
    assert p.shape == (1, 2) and s.shape == (1, 2, 3)
    launches = b.profile()['k_region_decode'][1]
    assert launches == 1
    bad = [((r + 1, 1), okq, 3, {}, 'restart range'), ((-1, 1), okq, 3, {}, 'restart range'), ((r, 0), okq, 3, {}, 'restart range'),
           ((r, 1), [], 3, {}, 'no queries'), ((r, 1), okq, 3, {'nq': -1}, 'no queries'),
           ((r, 1), okq, 3, {'null': 'out'}, 'no output'), ((r, 1), okq, 3, {'null': 'states'}, 'no output'),
           ((r, 1), okq, 0, {}, 'max_len'), ((r, 1), okq, -1, {}, 'max_len'), ((r, 1), okq, 16385, {}, 'max_len'), ((r, 1), okq, 2 ** 31 - 1, {}, 'max_len'),
           ((r, 1), okq, 2, {}, 'longer than max_len'), ((r, 1), okq + [[0, e0, -1, -1]], e0, {}, 'longer than max_len'),
           ((r, 1), [[2, 1, 0, 0]], 3, {}, 'first <= last'), ((r, 1), [[-1, 1, 0, 0]], 3, {}, 'first <= last'), ((r, 1), [[N - 1, N, 0, 0]], 3, {}, 'first <= last'),
           ((r, 1), [[e0 - 1, s1, 0, 0]], 3, {}, 'chain end'),
           ((r, 1), [[0, 2, len(MASKS), 0]], 3, {}, 'mask index'), ((r, 1), [[0, 2, -2, 0]], 3, {}, 'mask index'),
           ((r, 1), [[0, 2, 0, len(LABELS)]], 3, {}, 'label index'), ((r, 1), [[0, 2, 0, -2]], 3, {}, 'label index'),
           ((r, 1), okq, 3, {'null': 'masks'}, 'tables'), ((r, 1), okq, 3, {'null': 'labels'}, 'tables')]
    for (r0, nr), q, max_len, kw, text in bad:
        assert _c_call(b, r0, nr, q, masks, labels, constrain, max_len, states, out, **kw) == bpmodel.RMX_EARG, (q, max_len, kw, text)
        assert untouched(), (q, max_len, kw, text)                           # both output buffers are untouched
        assert re.search(text, hip._lib.load().rmx_last_error().decode()), (text, hip._lib.load().rmx_last_error())
        assert bpmodel.last_error_restarts() == []
        assert b.profile()['k_region_decode'][1] == launches, (q, max_len, kw)      # nothing was launched
    # valid at the edges: max_len exactly the longest query, a whole chain, max_len 16384
    assert _c_call(b, r, 1, okq + [[0, e0, -1, -1]], masks, labels, constrain, e0 + 1, states, out) == 0
    assert not np.isnan(out[:3]).any() and (out[:3] <= 0).all() and (out[3:] == -7.).all()
    assert (states[:3 * (e0 + 1)].reshape(3, -1)[2] >= 0).all() and (states[3 * (e0 + 1):] == -9).all()
    big = np.full(16384, -9, dtype=np.int16)
    assert _c_call(b, r, 1, okq[1:], masks, labels, constrain, 16384, big, out) == 0 and big[0] >= 0 and (big[1:] == -1).all()
    b.profile_enable(0)
    with pytest.raises(ValueError, match='^bad argument: .*mask index'):      # an index without a table
        b.region_decode_raw(r, 1, okq, None, labels, constrain)
    for kw in (dict(queries=[[0, 1, 0]]), dict(masks=masks[:, :, :-1]), dict(labels=labels[:1, :, :-1]), dict(constrain=np.ones(N + 1))):
        args = dict(queries=okq, masks=masks, labels=labels, constrain=None); args.update(kw)
        with pytest.raises(ValueError, match='must have shape'):
            b.region_decode_raw(r, 1, **args)
    for bad_call in (lambda: m.region_call([(0, 30)]), lambda: m.region_call([(0, 1)], ('nothing', None)), lambda: m.region_call([(3, 2)])):
        with pytest.raises(ValueError):
            bad_call()


def test_region_call_public_forms(hip, cases):
    """region_call on BreakpointModel and RestartSet against batch_region_calls over the twin."""
    from remixt_amd.restarts import RestartSet
    case = cases[GRIDS[0]]
    m = case.m
    regions = [(0, 9), (5, 5), (10, 40), (0, m.N - 1)]
    tb = _twin_batch(case)
    call = _call_states(case)
    for event in (None, ('not_loh', None), (None, 'state'), ('not_subclonal', 'unphased')):
        got = m.region_call(regions, event)
        want = posteriors.batch_region_calls(tb, 0, 1, regions, m.seg_fwd_remap, m.seg_is_original, m.is_telomere, event=event, cn=call[None])
        _check_region_call(got, want, regions, m, case, call, event, 'model, event %s' % (event,))
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=4, num_chains=3, seed=4)
    ps = synthetic.make_init_params(e, 2, 4)
    rs = RestartSet(e, ps, 4, num_clones=3, quiet=True, seeds=[0, 1])
    try:
        rs.variational_update(2)
        regions = [(0, 5), (12, 30), (39, 39)]
        res = rs.results()
        got = rs.region_call(regions, (None, 'total'), [x['cn'] for x in res])
        dec = rs.region_call(regions, (None, 'total'))
        for r in range(2):
            c = Case(rs.models[r])
            st = posteriors.states_in_model_order(res[r]['cn'], rs.batch, rs.models[r].seg_fwd_remap)
            want = posteriors.batch_region_calls(_twin_batch(c), 0, 1, regions, rs.models[r].seg_fwd_remap, rs.models[r].seg_is_original,
                                                 rs.models[r].is_telomere, event=(None, 'total'), cn=st[None])
            one = dict((k, v[r]) for k, v in got.items())
            _check_region_call(one, want, regions, rs.models[r], c, st, (None, 'total'), 'set, restart %d' % r)
            assert np.array_equal(dec['log_prob'][r], got['log_prob'][r])
    finally:
        rs.close()


def test_pipeline_cn_region_calls(hip, tmp_path):
    from remixt_amd import restarts, workflow
    from remixt_amd.analysis import pipeline
    from remixt_amd.restarts import RestartSet
    import pickle
    e, config, init_params = _pipeline_case()
    ids = sorted(init_params)
    seeds = [100 + i for i in ids]
    N = len(e.x)
    cn_regions = [('head', 0, 9), ('one', 50, 50), ('arm', 100, 299), ('genome', 0, N - 1)]
    R = len(cn_regions)
    config = dict(config, cn_regions=cn_regions)
    on_cfg = dict(config, cn_region_calls=True)
    keys = posteriors.REGION_CALL_ARRAYS
    base = pipeline.fit_restarts(e, init_params, config, seeds=seeds, groups=1)
    off = pipeline.fit_restarts(e, init_params, dict(config, cn_region_calls=False), seeds=seeds, groups=1)
    on = pipeline.fit_restarts(e, init_params, on_cfg, seeds=seeds, groups=1)
    # off: nothing of it in the results (they equal the ones without the key); on: the same results plus region_calls
    assert not any('region_calls' in res for res in list(base.values()) + list(off.values()))
    plain = lambda results: dict((i, dict((k, v) for k, v in res.items() if k != 'region_calls')) for i, res in results.items())
    cmp_ = lambda a, b: _same_results(dict((i, dict((k, v) for k, v in r.items() if k != 'region_events')) for i, r in a.items()),
                                      dict((i, dict((k, v) for k, v in r.items() if k != 'region_events')) for i, r in b.items()))
    cmp_(base, off)
    cmp_(base, plain(on))
    for i in ids:
        assert sorted(on[i]) == sorted(list(base[i]) + ['region_calls'])
        for k in posteriors.REGION_ARRAYS:
            assert np.array_equal(base[i]['region_events'][k], on[i]['region_events'][k]) and np.array_equal(base[i]['region_events'][k], off[i]['region_events'][k])
    with pytest.raises(ValueError, match='cn_regions'):
        pipeline.fit_restarts(e, init_params, dict(on_cfg, cn_regions=None), seeds=seeds, groups=1)
    # recomputation from the same fit
    rs = RestartSet(e, [init_params[i] for i in ids], 4, num_clones=3, quiet=True, seeds=seeds, **pipeline._model_kwargs(e, config))
    rs.fit(config['num_em_iter'], config['num_update_iter'])
    want = rs.region_call([r[1:] for r in cn_regions], None, [x['cn'] for x in rs.results()])
    rs.close()
    for j, i in enumerate(ids):
        rc = on[i]['region_calls']
        assert rc['names'] == [r[0] for r in cn_regions]
        for k in keys:
            assert rc[k].shape == (R,) and np.array_equal(rc[k], np.asarray(want[k][j], dtype=float)), (i, k)
        # the regional configuration is at least as probable as the call over the region's real segments ... up to the inserted
        # segments it also fixes; where the two agree everywhere and the region holds no inserted segment they are the same path
        assert (rc['log_prob'] <= 0).all() and (rc['log_prob_call'] <= 0).all() and (rc['n_differ'] >= 0).all()
    # pipeline.fit carries the same keys
    one = pipeline.fit(e, init_params[ids[1]], on_cfg, quiet=True, init_id=ids[1])
    assert sorted(one['region_calls']) == sorted(('names',) + keys) and one['region_calls']['log_prob'].shape == (R,)
    assert 'region_calls' not in pipeline.fit(e, init_params[ids[1]], config, quiet=True, init_id=ids[1])
    # the distributed form: the arrays through the record (one group, as fit_restarts ran above: the same fits to the bit)
    dist1 = restarts.fit_restarts_distributed(e, [init_params[i] for i in ids], 4, num_clones=3, num_em_iter=config['num_em_iter'],
                                              num_update_iter=config['num_update_iter'], seeds=seeds, quiet=True, groups=1, cn_regions=cn_regions,
                                              cn_region_calls=True, **pipeline._model_kwargs(e, config))
    for j, i in enumerate(ids):
        for k in keys:
            assert np.array_equal(dist1[j]['region_calls'][k], on[i]['region_calls'][k]), (i, k)
    # the workflow (fit_restarts_distributed + collate): the arrays in the store
    exp_file = str(tmp_path / 'experiment.pickle')
    with open(exp_file, 'wb') as f:
        pickle.dump(e, f)
    workflow.fit_model(exp_file, str(tmp_path / 'r.store'), on_cfg, None, seeds=seeds)
    with pipeline._Store(str(tmp_path / 'r.store'), 'r') as st:
        for i in sorted(st['stats']['init_id']):
            for k in keys:
                v = np.asarray(st['solutions/solution_%d/region_call_%s' % (i, k)])
                assert v.shape == (R,) and np.isfinite(v).all()
    workflow.fit_model(exp_file, str(tmp_path / 'r0.store'), config, None, seeds=seeds)
    with pipeline._Store(str(tmp_path / 'r0.store'), 'r') as st:
        assert not any('region_call_' in k for k in st.keys())
