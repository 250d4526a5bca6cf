"""Region alternatives on the device (rmx_region_kbest / k_region_kbest): against the log-domain numpy twin on the read-back
framelogprob / log_transmat, identities on the device alone, state classes, the mixed-model state, inserted segments, invariance
to batching, grouping, padding, K and chunking, no side effects on the model, refusals and the public forms.

Tolerance: the family's bound, L 1e-9 in log P for a run of L segments.  Paths are not compared with the
twin's paths for equality -- rounding-level near-ties exist on real fits -- but through their own probability: for
every query and rank k
  1. a returned path satisfies the event exactly, entries past the run are -1, and the paths of a query are pairwise distinct;
  2. the values do not increase, beyond 2 L 1e-9;
  3. |log P*_k - twin log-probability of the returned path k| <= L 1e-9;
  4. twin log-probability of path k >= the twin's k-th optimum - 2 L 1e-9;
  5. a rank is -inf exactly where the twin's is, and then its states are -1.
The fits, runs and constraints are those of tests/test_hip_region_decode.py (60 segments at 165 states, 40 at 355, 24 at 457: both
adjacency kinds, a strided s, and with K in {1, 3, 8} the list lengths 1, 4 and 8; K = 2 runs in test_invariance)."""
import ctypes as C
import re

import numpy as np
import pytest

from remixt_amd import posteriors, synthetic
from tests import decode_twin, kbest_twin
from tests import helpers as H
from tests.test_hip_region_decode import BOUND, BP_BUDGET, OUT_BUDGET, U, _call_states, _inserted_model, _path_logprob, _queries, _runs, _tables
from tests.test_hip_region_events import LABELS, MASKS, Case
from tests.test_hip_region_pattern import _longest
from tests.test_hip_region_span import CHAINS, CONSTRAINTS
from tests.test_hip_sample_cn import GRIDS, _fitted, _model_state

pytestmark = pytest.mark.gpu

KS = (1, 3, 8)
KMAX = 8


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


def _raw(case, runs, K, constraints=CONSTRAINTS, r0=None, nr=1, max_len=None):
    logp, states = case.b.region_kbest_raw(case.r if r0 is None else r0, nr, _queries(runs, constraints), K, case.masks, case.labels, case.constrain, max_len)
    return logp.reshape(nr, len(runs), len(constraints), K), states.reshape(nr, len(runs), len(constraints), K, -1)


def _want(case, runs, constraints=CONSTRAINTS):
    """The twin's lists at K = 8 (its ranks below K' are its K'-list: the stable sort keeps prefixes)."""
    return [[kbest_twin.kbest(case.twin, a, b, KMAX, *_tables(case, mk, lb), case.constrain) for mk, lb in constraints] for a, b in runs]


def _check(case, runs, logp, states, want, K, tag, constraints=CONSTRAINTS):
    """The five checks of the module docstring for one restart's results; returns (finite ranks, all ranks)."""
    worst, finite = 0., 0
    for i, (a, b) in enumerate(runs):
        L = b - a + 1
        for j, (mk, lb) in enumerate(constraints):
            g, st, (w, _) = logp[i, j], states[i, j], want[i][j]
            what = (tag, a, b, mk, lb)
            assert not np.isnan(g).any(), what
            assert np.array_equal(g == -np.inf, w[:K] == -np.inf), what + (g, w[:K])
            assert (st[:, L:] == -1).all(), what
            found = int(np.isfinite(g).sum())
            assert np.isfinite(g[:found]).all() and (st[found:] == -1).all(), what
            assert (np.diff(g[:found]) <= 2 * L * BOUND).all(), what + (g,)
            assert len(set(tuple(p) for p in st[:found, :L])) == found, what           # pairwise distinct
            mask, label = _tables(case, mk, lb)
            for k in range(found):
                finite += 1
                assert (st[k, :L] >= 0).all() and (st[k, :L] < case.S).all()
                assert decode_twin.satisfies(st[k, :L], a, b, mask, label, case.constrain), what + (k, st[k, :L])
                own = _path_logprob(case, a, b, st[k, :L])
                e3, e4 = abs(g[k] - own) / (L * BOUND), (w[k] - own) / (2 * L * BOUND)
                worst = max(worst, e3, e4)
                assert e3 <= 1., what + (k, g[k], own)
                assert e4 <= 1., what + (k, own, w[k])
            print('%s run [%d, %d] mask %s label %s: log P*_k %s, twin optima %s' % (tag, a, b, mk, lb, g, w[:K]))
    print('%s K %d: worst error / bound %.3e over %d finite ranks of %d' % (tag, K, worst, finite, len(runs) * len(constraints) * K))
    return finite, len(runs) * len(constraints) * K


class KbestCase(Case):
    def __init__(self, m, **kw):
        Case.__init__(self, m, **kw)
        self.runs = _runs(self)
        self.want = _want(self, self.runs)      # (computed once, shared by the tests of the grid)


@pytest.fixture(scope='module')
def cases(hip):
    return dict(((N, M, c), KbestCase(_fitted(hip, N, M, c, chains=CHAINS[c]))) for N, M, c in GRIDS)


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_twin(hip, cases, N, M, max_cn, K):
    case = cases[(N, M, max_cn)]
    assert case.S == {8: 165, 12: 355, 6: 457}[max_cn] and case.S % 64
    logp, states = _raw(case, case.runs, K)
    assert states.shape[-2:] == (K, max(z - a + 1 for a, z in case.runs)) and states.dtype == np.int16
    finite, total = _check(case, case.runs, logp[0], states[0], case.want, K, 'S %d' % case.S)
    assert finite >= total // (2 * K)
    # the model-level form
    q = _queries(case.runs)
    one_p, one_s = case.m.model.region_kbest(q, K, case.masks, case.labels, case.constrain)
    assert one_p.shape == (len(q), K) and np.array_equal(one_p, logp[0].reshape(len(q), K)) and np.array_equal(one_s, states[0].reshape(len(q), K, -1))


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_identities(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    b, S, r = case.b, case.S, case.r
    q = _queries(case.runs)
    Lq = (q[:, 1] - q[:, 0] + 1).astype(float)
    dec_p, dec_s = b.region_decode_raw(r, 1, q, case.masks, case.labels, case.constrain)
    lists = {}
    for K in KS:
        lp, st = b.region_kbest_raw(r, 1, q, K, case.masks, case.labels, case.constrain)
        lists[K] = (lp[0], st[0])
        # rank 0 equals region_decode_raw, value and path, bit for bit
        assert np.array_equal(lp[0, :, 0], dec_p[0]) and np.array_equal(st[0, :, 0], dec_s[0]), K
    logp, states = lists[KMAX]
    fin = np.isfinite(logp)
    # every rank equals call_logprob_raw of its own path (label -1, every segment binds)
    paths = np.zeros((1, len(q) * KMAX, case.N), dtype=np.int16)
    for i, k in zip(*np.nonzero(fin)):
        paths[0, i * KMAX + k, q[i, 0]:q[i, 1] + 1] = states[i, k, :int(Lq[i])]
    qc = np.array([[q[i, 0], q[i, 1], -1, i * KMAX + k] for i in range(len(q)) for k in range(KMAX)], dtype=np.int32)
    own = b.call_logprob_raw(r, 1, paths, qc, case.labels, None)[0].reshape(len(q), KMAX)
    err = np.abs(logp[fin] - own[fin]) / np.broadcast_to(Lq[:, None], logp.shape)[fin]
    assert (err <= BOUND).all(), err.max()
    # the list does not exceed the sum
    total = b.region_logprob_raw(r, 1, q, case.masks, case.labels, case.constrain)[0]
    with np.errstate(divide='ignore'):
        lse = np.logaddexp.reduce(logp, axis=1)
    assert np.array_equal(total == -np.inf, ~fin[:, 0]) and (lse[fin[:, 0]] <= total[fin[:, 0]] + Lq[fin[:, 0]] * BOUND).all()
    print('S %d: max |log P*_k - call_logprob of its path| / L %.3e; the lists hold %.4f .. %.4f of their events' % (
        S, err.max(), np.exp(lse - total)[fin[:, 0]].min(), np.exp(lse - total)[fin[:, 0]].max()))
    # a one-segment query: its ranks are the K largest masked read-back marginals in numpy's stable order, exactly
    post = b.get_array(r, 'posterior_marginals')
    ns = np.arange(case.N)
    for k in (None,) + tuple(MASKS):
        q1 = np.array([[n, n, -1 if k is None else MASKS.index(k), -1] for n in ns], dtype=np.int32)
        lp, st = b.region_kbest_raw(r, 1, q1, KMAX, case.masks, case.labels, case.constrain)
        row = post if k is None else np.where(case.mask_seg[k] | ~case.constrain[:, None], post, 0.)
        order = np.argsort(-row, axis=1, kind='stable')[:, :KMAX]
        top = np.take_along_axis(row, order, axis=1)
        assert st.shape == (1, case.N, KMAX, 1)
        assert np.array_equal(st[0, :, :, 0], np.where(top > 0, order, -1)), k
        ok = top > 0
        assert np.array_equal(lp[0] == -np.inf, ~ok), k
        tol = ((S + 4) + 3 * np.abs(np.log(top[ok]))) * U      # (k_region_decode's one-segment tolerance: the read-back row and one logarithm)
        assert (np.abs(np.exp(lp[0][ok]) / top[ok] - 1) <= tol).all(), k
    # a mask that admits one state per class: one finite rank, the others -inf
    call = _call_states(case)
    c0, c1 = _longest(case)
    s0 = int(np.bincount(call[c0:c0 + 10], minlength=S).argmax())
    one = np.zeros((b.cn_classes.shape[0], 1, S), dtype=np.uint8); one[:, 0, s0] = 1
    q1 = np.array([[c0, c0 + 9, 0, -1], [c0 + 2, c0 + 2, 0, -1]], dtype=np.int32)
    lp1, st1 = b.region_kbest_raw(r, 1, q1, KMAX, one, None, None)
    assert np.isfinite(lp1[0, :, 0]).all() and (lp1[0, :, 1:] == -np.inf).all() and (st1[0, :, 1:] == -1).all()
    assert (st1[0, 0, 0] == s0).all() and st1[0, 1, 0, 0] == s0 and (st1[0, 1, 0, 1:] == -1).all()
    # no sampled path that satisfies the event, and is not in the list, beats the last rank by more than the bound
    K = 256
    smp = b.sample_states(r, 1, K, [11])                                   # (1, K, N)
    sel = [i for i in range(len(q)) if fin[i, 0] and Lq[i] > 1]
    qs = np.array([[q[i, 0], q[i, 1], -1, k] for i in sel for k in range(K)], dtype=np.int32)
    lps = b.call_logprob_raw(r, 1, smp.astype(np.int16), qs, None, None)[0].reshape(len(sel), K)
    hits = inlist = 0
    for row, i in enumerate(sel):
        a, z = int(q[i, 0]), int(q[i, 1])
        mk, lb = CONSTRAINTS[i % len(CONSTRAINTS)]
        mask, label = _tables(case, mk, lb)
        mine = set(tuple(p) for p in states[i, :, :z - a + 1])
        for k in range(K):
            sub = smp[0, k, a:z + 1]
            if decode_twin.satisfies(sub, a, z, mask, label, case.constrain):
                hits += 1
                if tuple(sub) in mine:
                    inlist += 1
                else:
                    assert lps[row, k] <= logp[i, KMAX - 1] + Lq[i] * BOUND, (a, z, mk, lb, k, lps[row, k], logp[i])
    assert hits > 0
    print('S %d: %d sampled sub-paths satisfy their event, %d of them in the lists, none of the others above rank %d' % (S, hits, inlist, KMAX - 1))


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
        b.set_array(0, 'allele_likelihood_mask', np.zeros(N, dtype=np.int64))
        b.variational_update(2)
        case = Case(m, batch=b, r=0)
        loh = case.masks[:, MASKS.index('loh')]
        assert not loh[0].any() and loh[1].any()                         # the mask differs per class
        runs = _runs(case)[:4]
        logp, states = _raw(case, runs, 3)
        _check(case, runs, logp[0], states[0], _want(case, runs), 3, 'two classes')
        # LOH is possible only at the odd segments: a run of two is impossible, an odd segment alone is not
        odd = [n for n in range(3, N - 2, 2) if case.tel[n - 1] == 0 and case.tel[n] == 0]
        lp, st = _raw(case, [(n, n) for n in odd] + [(n, n + 1) for n in odd], 3, [('loh', None)])
        assert np.isfinite(lp[0, :len(odd), 0, 0]).all() and np.isneginf(lp[0, len(odd):, 0]).all() and (st[0, len(odd):] == -1).all()
        assert all(loh[1][s] for s in st[0, :len(odd), 0, 0, 0])
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
        K = 3
        call = lambda r0, nr: b.region_kbest_raw(r0, nr, q, K, case.masks, case.labels, case.constrain)
        full_p, full_s = call(0, 4)
        assert len(np.unique(full_p[:, :, 0], axis=0)) > 1
        dec_p, dec_s = b.region_decode_raw(0, 4, q, case.masks, case.labels, case.constrain)
        assert np.array_equal(full_p[:, :, 0], dec_p) and np.array_equal(full_s[:, :, 0], dec_s)
        for r in range(4):
            p, s = call(r, 1)
            assert np.array_equal(p[0], full_p[r]) and np.array_equal(s[0], full_s[r]), r
        p, s = call(1, 3)
        assert np.array_equal(p, full_p[1:]) and np.array_equal(s, full_s[1:])
        for cs_ in cases:
            shape = (len(runs), len(CONSTRAINTS), K)
            _check(cs_, runs, full_p[cs_.r].reshape(shape), full_s[cs_.r].reshape(shape + (-1,)), _want(cs_, runs), K, 'mixed model, restart %d' % cs_.r)
    finally:
        rs.close()


def _twin_batch(case):
    return kbest_twin.KbestTwinBatch(case.b.cn_classes, case.b.seg_class, [case.b.get_array(case.r, 'framelogprob')],
                                     [case.b.get_array(case.r, 'log_transmat')], case.cs, case.ce)


def _check_alternatives(got, want, regions, m, case, call_states, tag):
    """region_alternatives' list over regions of one restart against batch_region_alternatives over the twin."""
    runs, piece_region, _ = posteriors.region_queries(np.array([r[-2:] for r in regions]), m.seg_fwd_remap, m.seg_is_original, case.cs, case.ce)
    fwd = np.asarray(m.seg_fwd_remap)
    assert len(got) == len(regions)
    for k, (g, w) in enumerate(zip(got, want)):
        Lk = float(sum(z - a + 1 for (a, z), p in zip(runs, piece_region) if p == k))
        K = len(g['log_prob'])
        assert np.array_equal(np.isfinite(g['log_prob']), np.isfinite(w['log_prob'])), (tag, k)
        found = len(g['cn'])
        assert found == int(np.isfinite(g['log_prob']).sum()) == len(w['cn'])
        print('%s region %s: log_prob %s (twin %s), coverage %.6f, rank of call %d, duplicates %s' % (
            tag, regions[k], g['log_prob'], w['log_prob'], g['coverage'], g['rank_of_call'], g['duplicate_of']))
        assert (np.abs(g['log_prob'][:found] - w['log_prob'][:found]) <= 2 * Lk * BOUND).all(), (tag, k)
        assert abs(g['log_p_event'] - w['log_p_event']) <= 2 * Lk * BOUND
        assert np.array_equal(g['log_prob_given_event'][:found], g['log_prob'][:found] - g['log_p_event'])
        assert abs(g['coverage'] - np.exp(g['log_prob_given_event'][:found]).sum()) <= 1e-12 and g['coverage'] <= 1 + 2 * K * Lk * BOUND
        seg = fwd[regions[k][-2]:regions[k][-1] + 1]
        own = []
        for rank in range(found):
            assert g['cn'][rank].shape == (len(seg), 3, 2)
            own.append(np.array([int(np.flatnonzero((case.b.cn_classes[case.b.seg_class[n]] == g['cn'][rank][i]).all(axis=(1, 2)))[0]) for i, n in enumerate(seg)]))
            assert g['n_differ'][rank] == (own[rank] != call_states[seg]).sum()
            same = [j for j in range(rank) if np.array_equal(own[j], own[rank])]
            assert g['duplicate_of'][rank] == (same[0] if same else -1)
        hits = [rank for rank in range(found) if g['n_differ'][rank] == 0]
        assert g['rank_of_call'] == (hits[0] if hits else -1)
        assert (g['n_differ'][found:] == -1).all() and (g['duplicate_of'][found:] == -1).all()


def test_inserted_segments(hip):
    """Two breakends on one boundary: the model inserts a zero-length segment there.  A mask does not bind it, a label binds the
    adjacencies through it, its state is part of a configuration: two paths that differ only there are two ranks with the same
    copy numbers on the region's own segments, kept and marked."""
    m = _inserted_model(hip)
    case = Case(m)
    assert m.N1 > m.N and not case.constrain.all()
    dummy = int(np.flatnonzero(~case.constrain & (np.arange(m.N1) > 0) & (case.tel == 0))[0])
    runs = [(dummy - 1, dummy + 1), (dummy, dummy), (dummy, dummy + 1), (dummy - 3, dummy + 2)]
    logp, states = _raw(case, runs, KMAX)
    _check(case, runs, logp[0], states[0], _want(case, runs), KMAX, 'inserted segment')
    i = int(m.seg_rev_remap[dummy - 1])
    fwd = np.asarray(m.seg_fwd_remap)
    assert fwd[i] == dummy - 1 and fwd[i + 1] == dummy + 1
    regions = [(i, i + 1), (i - 2, i), (i + 1, i + 1), (0, 2), (m.N - 2, m.N - 1), (0, m.N - 1)]
    tb = _twin_batch(case)
    call = _call_states(case)
    for event in (None, ('not_subclonal', None), (None, 'total'), ('not_loh', 'total')):
        got = m.region_alternatives(regions, KMAX, event)
        want = posteriors.batch_region_alternatives(tb, 0, 1, regions, m.seg_fwd_remap, m.seg_is_original, m.is_telomere, k=KMAX, event=event, cn=call[None])[0]
        _check_alternatives(got, want, regions, m, case, call, 'event %s' % (event,))
    # region (i, i + 1) holds the inserted segment: the S states it can take give paths with one pair of copy numbers; the
    # device's own paths show it (distinct state paths, equal on the two original segments), and the public form marks it
    got = m.region_alternatives([(i, i + 1)], KMAX)[0]
    lp, st = _raw(case, [(dummy - 1, dummy + 1)], KMAX, [(None, None)])
    st = st[0, 0, 0]
    pairs = [(j, k) for k in range(KMAX) for j in range(k) if st[j, 0] == st[k, 0] and st[j, 2] == st[k, 2]]
    print('inserted segment %d: paths %s, duplicate_of %s' % (dummy, st[:, :3].tolist(), got['duplicate_of']))
    assert pairs and all(st[j, 1] != st[k, 1] for j, k in pairs)
    assert (got['duplicate_of'] >= 0).any()
    for k in np.flatnonzero(got['duplicate_of'] >= 0):
        assert np.array_equal(got['cn'][k], got['cn'][got['duplicate_of'][k]]) and got['log_prob'][k] <= got['log_prob'][got['duplicate_of'][k]]


def _plan(nr, nq, S, K, max_len):
    """rmxh::kbest_plan (remixt_amd/csrc/rmx_host.h): (restarts per block, queries per chunk)."""
    strip_bytes, per_out = 2 * S * K * max_len, K * (8 + 2 * max_len)
    strips = max(1, BP_BUDGET // strip_bytes)
    nrc = min(nr, 65535, strips, max(1, (OUT_BUDGET - 24) // per_out))
    return nrc, max(1, min(nq, strips // nrc, (OUT_BUDGET - 8) // (nrc * per_out + 16)))


def test_invariance(hip, cases):
    """A (restart, query) result, all K values and paths, is bit-identical in any restart range, any batch and order of queries,
    for any max_len, in any K that covers the rank, across RestartSet / RestartGroups, and in a call that runs in several chunks."""
    from remixt_amd.restarts import RestartGroups, RestartSet
    e = synthetic.make_experiment(80, num_clones=3, max_copy_number=4, num_chains=3, seed=4)
    ps = synthetic.make_init_params(e, 4, 4)
    rs = RestartSet(e, ps, 4, num_clones=3, quiet=True, seeds=list(range(4)))
    rs.variational_update(2)
    b, m = rs.batch, rs.models[0]
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
    call = lambda r0, nr, qq, K=KMAX, ml=None: b.region_kbest_raw(r0, nr, qq, K, masks, labels, constrain, ml)
    full_p, full_s = call(0, 4, q)
    assert full_p.shape == (4, len(q), KMAX) and full_s.shape == (4, len(q), KMAX, longest) and not np.isnan(full_p).any()
    assert not np.array_equal(full_p[0], full_p[1]) and 2 * np.isfinite(full_p[:, :, 0]).sum() >= full_p[:, :, 0].size
    for r in range(4):
        p, s = call(r, 1, q)
        assert np.array_equal(p[0], full_p[r]) and np.array_equal(s[0], full_s[r])
    p, s = call(1, 2, q)
    assert np.array_equal(p, full_p[1:3]) and np.array_equal(s, full_s[1:3])
    # the prefix property: ranks 0 .. K' - 1 of the K = 8 call are the K' call, for every K' (every list length)
    for K in range(1, KMAX):
        p, s = call(0, 4, q, K)
        assert p.shape == (4, len(q), K) and np.array_equal(p, full_p[:, :, :K]) and np.array_equal(s, full_s[:, :, :K]), K
    # single queries (max_len: that query's own length), and the queries in another order
    for i in range(0, len(q), 5):
        p, s = call(0, 4, q[i:i + 1])
        L = int(q[i, 1] - q[i, 0] + 1)
        assert s.shape[3] == L and np.array_equal(p[:, 0], full_p[:, i]) and np.array_equal(s[:, 0], full_s[:, i, :, :L])
    p, s = call(0, 4, q[::-1].copy())
    assert np.array_equal(p, full_p[:, ::-1]) and np.array_equal(s, full_s[:, ::-1])
    # padding: max_len 1024 against the longest query
    p, s = call(0, 4, q, KMAX, 1024)
    assert s.shape == (4, len(q), KMAX, 1024) and np.array_equal(p, full_p) and np.array_equal(s[..., :longest], full_s) and (s[..., longest:] == -1).all()
    # the public forms: one restart of a set, and groups against one group
    regions = [(4, 12), (20, 20), (0, 1), (30, 60)]
    for event in (None, ('not_loh', 'total')):
        per_set, one = rs.region_alternatives(regions, 4, event), rs.models[2].region_alternatives(regions, 4, event)
        assert len(per_set) == 4 and _same_alternatives(per_set[2], one)
    rs.close()
    groups = RestartGroups(e, ps, 4, groups=2, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    single = RestartGroups(e, ps, 4, groups=1, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    for g in (groups, single):
        g.variational_update(2)
    x, y = groups.region_alternatives(regions, 4, ('not_loh', 'total')), single.region_alternatives(regions, 4, ('not_loh', 'total'))
    assert len(x) == len(y) == 4 and all(_same_alternatives(u, v) for u, v in zip(x, y))
    groups.close(); single.close()
    # several chunks on the 60-segment fit: at K = 8 and max_len 16384 a strip is 16384 * 8 * 165 int16, and rmxh::kbest_plan
    # gives chunks of `qc` queries for one restart
    case = cases[GRIDS[0]]
    q = _queries(case.runs)
    nrc, qc = _plan(1, len(q), case.S, KMAX, 16384)
    assert nrc == 1 and 1 <= qc < len(q) and -(-len(q) // qc) >= 2, (nrc, qc, len(q))
    one_p, one_s = case.b.region_kbest_raw(case.r, 1, q, KMAX, case.masks, case.labels, case.constrain)
    assert _plan(1, len(q), case.S, KMAX, one_s.shape[-1]) == (1, len(q))                  # (that call ran in one chunk)
    p, s = case.b.region_kbest_raw(case.r, 1, q, KMAX, case.masks, case.labels, case.constrain, 16384)
    L = one_s.shape[-1]
    print('%d queries at K 8, max_len 16384, %d states: %d chunks of %d' % (len(q), case.S, -(-len(q) // qc), qc))
    assert np.array_equal(p, one_p) and np.array_equal(s[..., :L], one_s) and (s[..., L:] == -1).all()


def _same_alternatives(x, y):
    """Two lists over regions of region_alternatives' dicts, bit for bit."""
    if len(x) != len(y):
        return False
    for u, v in zip(x, y):
        if sorted(u) != sorted(v) or len(u['cn']) != len(v['cn']) or not all(np.array_equal(a, b) for a, b in zip(u['cn'], v['cn'])):
            return False
        if not all(np.array_equal(np.asarray(u[k]), np.asarray(v[k]), equal_nan=True) for k in u if k != 'cn'):
            return False
    return True


def _query_bits():
    """tools/query_bits.py as a module (tools is not a package)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('query_bits', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'query_bits.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_no_side_effects(hip):
    """Every array of tools/query_bits.py's list of the other queries -- samples, posterior summary, region probabilities, counts,
    call probabilities, extents, patterns, decode, extremes, conditionals, moments, with and without unbound segments, four
    restarts of which two under the other transition model -- is the same before and after calls of region_kbest_raw that grow
    and overwrite the staging buffer, the table buffer and the back-pointer buffer those queries share; so is the model's state,
    and a fit continued after the calls equals one without them."""
    qb = _query_bits()
    rs = qb.open_scenario(*qb.GRIDS[0])
    try:
        b, m = rs.batch, rs.models[0]
        before, state = {}, _model_state(m)
        qb.collect(rs, before, kbest=False)
        assert len(before) >= 34 and not any('kbest' in k for k in before)
        masks, labels = posteriors.event_tables(b.cn_classes)
        cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
        q = np.array([[int(a), int(z), mi, li] for a, z in zip(cs, ce) for mi, li in ((-1, -1), (1, 0), (5, 2))], dtype=np.int32)
        for K, max_len in ((8, 4096), (3, None), (1, 64)):
            lp, st = b.region_kbest_raw(0, qb.R, q, K, masks, labels, np.asarray(m.seg_is_original, dtype=np.uint8), max_len)
            assert np.isfinite(lp[:, :, 0]).any()
        out = rs.region_alternatives([(0, 9), (20, 22), (40, 49)], 8, ('not_loh', 'state'))
        assert len(out) == qb.R and all((o['log_prob'][:len(o['cn'])] <= 0).all() for row in out for o in row)
        after = {}
        qb.collect(rs, after, kbest=False)
        assert sorted(before) == sorted(after)
        for k in before:
            assert before[k].dtype == after[k].dtype and np.array_equal(before[k], after[k], equal_nan=before[k].dtype.kind == 'f'), k
        again = _model_state(m)
        for k in state:
            assert np.array_equal(state[k], again[k], equal_nan=True), k
    finally:
        rs.close()
    # a fit continued after the calls equals one without them
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    out = m1.region_alternatives([(0, 49)], 3)
    assert len(out[0]['cn']) == 3 and out[0]['n_differ'][0] >= 0
    for m in (m1, m2):
        m.variational_update()
        m.variational_update()
    s1, s2 = _model_state(m1), _model_state(m2)
    for k in s1:
        assert np.array_equal(s1[k], s2[k], equal_nan=True), k
    assert m1.model.calculate_elbo() == m2.model.calculate_elbo()


def test_large_state_count(hip):
    """951 states: at K = 8 the kernel's dynamic LDS is 952 * 78 = 74 256 bytes, above the 64 KiB a launch gets without the raised
    limit (K = 4: 43 792 bytes, below it), and a thread owns four states.  Identities on the device alone: rank 0 equals
    region_decode_raw bit for bit, ranks 0 .. 3 of K = 8 equal the K = 4 call, every rank is call_logprob_raw of its own path
    within the bound, paths are pairwise distinct and values do not increase."""
    m = _fitted(hip, 16, 3, 20, chains=2)
    case = Case(m)
    assert case.S == 951 and ((case.S + 3) // 4 * 4) * (8 * 8 + 14) > 64 * 1024
    c = int(np.argmax(case.ce - case.cs))
    c0, c1 = int(case.cs[c]), int(case.ce[c])
    assert c1 - c0 >= 4
    runs = [(c0, c1), (c0 + 1, c0 + 3), (c0 + 2, c0 + 2)]
    q = _queries(runs)
    Lq = (q[:, 1] - q[:, 0] + 1).astype(float)
    b, r = case.b, case.r
    dec_p, dec_s = b.region_decode_raw(r, 1, q, case.masks, case.labels, case.constrain)
    lp, st = b.region_kbest_raw(r, 1, q, 8, case.masks, case.labels, case.constrain)
    lp4, st4 = b.region_kbest_raw(r, 1, q, 4, case.masks, case.labels, case.constrain)
    assert np.array_equal(lp[0, :, 0], dec_p[0]) and np.array_equal(st[0, :, 0], dec_s[0])
    assert np.array_equal(lp[:, :, :4], lp4) and np.array_equal(st[:, :, :4], st4)
    fin = np.isfinite(lp[0])
    assert fin[:, 0].sum() * 2 >= len(q) and not np.isnan(lp).any()
    paths = np.zeros((1, len(q) * 8, case.N), dtype=np.int16)
    for i, k in zip(*np.nonzero(fin)):
        paths[0, i * 8 + k, q[i, 0]:q[i, 1] + 1] = st[0, i, k, :int(Lq[i])]
    qc = np.array([[q[i, 0], q[i, 1], -1, i * 8 + k] for i in range(len(q)) for k in range(8)], dtype=np.int32)
    own = b.call_logprob_raw(r, 1, paths, qc, case.labels, None)[0].reshape(len(q), 8)
    err = np.abs(lp[0][fin] - own[fin]) / np.broadcast_to(Lq[:, None], fin.shape)[fin]
    print('951 states: %d finite ranks, max |log P*_k - call_logprob of its path| / L %.3e' % (fin.sum(), err.max()))
    assert (err <= BOUND).all()
    for i in range(len(q)):
        found, L = int(fin[i].sum()), int(Lq[i])
        assert fin[i, :found].all() and (st[0, i, found:] == -1).all() and (st[0, i, :, L:] == -1).all()
        assert len(set(tuple(p) for p in st[0, i, :found, :L])) == found and (np.diff(lp[0, i, :found]) <= 2 * L * BOUND).all()


def _c_call(b, r, nr, q, masks, labels, constrain, K, max_len, states, out, null=None, nq=None):
    """rmx_region_kbest through ctypes with the caller's output buffers: the return code."""
    dp, ip, u8p, i16p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int16)
    q = np.ascontiguousarray(q, dtype=np.int32).reshape(-1, 4)
    masks, labels = np.ascontiguousarray(masks, dtype=np.uint8), np.ascontiguousarray(labels, dtype=np.int16)
    constrain = np.ascontiguousarray(constrain, dtype=np.uint8)
    return b._lib.rmx_region_kbest(b._handle, r, nr, len(q) if nq is None else nq, q.ctypes.data_as(ip) if len(q) else ip(),
                                   masks.shape[1], u8p() if null == 'masks' else masks.ctypes.data_as(u8p), labels.shape[1],
                                   i16p() if null == 'labels' else labels.ctypes.data_as(i16p), constrain.ctypes.data_as(u8p), K, max_len,
                                   i16p() if null == 'states' else states.ctypes.data_as(i16p), dp() if null == 'out' else out.ctypes.data_as(dp))


def test_refusals(hip):
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
    out, states = np.full(64, -7.), np.full(512, -9, dtype=np.int16)
    untouched = lambda: (out == -7.).all() and (states == -9).all()
    # before update_p_cn: RMX_EVALUE with the restart listed
    assert _c_call(b, r, 1, okq, masks, labels, constrain, 3, 3, states, out) == bpmodel.RMX_EVALUE and untouched()
    with pytest.raises(ValueError, match='update_p_cn'):
        b.region_kbest_raw(r, 1, okq, 3, masks, labels, constrain)
    assert bpmodel.last_error_restarts() == [r]
    m.variational_update()
    p, s = b.region_kbest_raw(r, 1, okq, 3, masks, labels, constrain)
    assert p.shape == (1, 2, 3) and s.shape == (1, 2, 3, 3)
    bad = [((r + 1, 1), okq, 3, 3, {}, 'restart range'), ((-1, 1), okq, 3, 3, {}, 'restart range'), ((r, 0), okq, 3, 3, {}, 'restart range'),
           ((r, 1), [], 3, 3, {}, 'no queries'), ((r, 1), okq, 3, 3, {'nq': -1}, 'no queries'),
           ((r, 1), okq, 3, 3, {'null': 'out'}, 'no output'), ((r, 1), okq, 3, 3, {'null': 'states'}, 'no output'),
           ((r, 1), okq, 0, 3, {}, r'K must be in \[1, 8\]'), ((r, 1), okq, -1, 3, {}, 'K must be'), ((r, 1), okq, 9, 3, {}, 'K must be'),
           ((r, 1), okq, 2 ** 31 - 1, 3, {}, 'K must be'), ((r, 1), okq, -2 ** 31, 3, {}, 'K must be'),
           ((r, 1), okq, 3, 0, {}, 'max_len'), ((r, 1), okq, 3, -1, {}, 'max_len'), ((r, 1), okq, 3, 16385, {}, 'max_len'), ((r, 1), okq, 3, 2 ** 31 - 1, {}, 'max_len'),
           ((r, 1), okq, 3, 2, {}, 'longer than max_len'), ((r, 1), okq + [[0, e0, -1, -1]], 3, e0, {}, 'longer than max_len'),
           ((r, 1), [[2, 1, 0, 0]], 3, 3, {}, 'first <= last'), ((r, 1), [[-1, 1, 0, 0]], 3, 3, {}, 'first <= last'), ((r, 1), [[N - 1, N, 0, 0]], 3, 3, {}, 'first <= last'),
           ((r, 1), [[e0 - 1, s1, 0, 0]], 3, 3, {}, 'chain end'),
           ((r, 1), [[0, 2, len(MASKS), 0]], 3, 3, {}, 'mask index'), ((r, 1), [[0, 2, -2, 0]], 3, 3, {}, 'mask index'),
           ((r, 1), [[0, 2, 0, len(LABELS)]], 3, 3, {}, 'label index'), ((r, 1), [[0, 2, 0, -2]], 3, 3, {}, 'label index'),
           ((r, 1), okq, 3, 3, {'null': 'masks'}, 'tables'), ((r, 1), okq, 3, 3, {'null': 'labels'}, 'tables')]
    for (r0, nr), q, K, max_len, kw, text in bad:
        assert _c_call(b, r0, nr, q, masks, labels, constrain, K, max_len, states, out, **kw) == bpmodel.RMX_EARG, (q, K, max_len, kw, text)
        assert untouched(), (q, K, max_len, kw, text)                       # both output buffers are untouched
        assert re.search(text, hip._lib.load().rmx_last_error().decode()), (text, hip._lib.load().rmx_last_error())
        assert bpmodel.last_error_restarts() == []
    # valid at the edges: K 1 and 8, max_len exactly the longest query, a whole chain
    assert _c_call(b, r, 1, okq + [[0, e0, -1, -1]], masks, labels, constrain, 8, e0 + 1, states, out) == 0
    assert not np.isnan(out[:24]).any() and (out[:24] <= 0).all() and (out[24:] == -7.).all() and (states[24 * (e0 + 1):] == -9).all()
    assert (states[:24 * (e0 + 1)].reshape(3, 8, -1)[2, 0] >= 0).all()
    out[:], states[:] = -7., -9
    assert _c_call(b, r, 1, okq, masks, labels, constrain, 1, 3, states, out) == 0 and (out[2:] == -7.).all() and (states[6:] == -9).all()
    assert np.array_equal(out[:2], p[0, :, 0]) and np.array_equal(states[:6].reshape(2, 3), s[0, :, 0])
    with pytest.raises(ValueError, match='K must be'):
        b.region_kbest_raw(r, 1, okq, 9, masks, labels, constrain)
    for bad_call in (lambda: m.region_alternatives([(0, 30)]), lambda: m.region_alternatives([(0, 1)], 4, ('nothing', None)),
                     lambda: m.region_alternatives([(3, 2)]), lambda: m.region_alternatives([(0, 1)], 0), lambda: m.region_alternatives([(0, 1)], 9)):
        with pytest.raises(ValueError):
            bad_call()


def test_region_alternatives_public_forms(hip, cases):
    """region_alternatives on BreakpointModel, RestartSet, RestartGroups and DatasetGroups against batch_region_alternatives over
    the twin."""
    from remixt_amd.restarts import DatasetGroups, RestartGroups, RestartSet
    case = cases[GRIDS[0]]
    m = case.m
    regions = [(0, 9), (5, 5), (10, 40), (0, m.N - 1)]
    tb = _twin_batch(case)
    call = _call_states(case)
    for event in (None, ('not_loh', None), (None, 'state'), ('not_subclonal', 'unphased')):
        got = m.region_alternatives(regions, 4, event)
        want = posteriors.batch_region_alternatives(tb, 0, 1, regions, m.seg_fwd_remap, m.seg_is_original, m.is_telomere, k=4, event=event, cn=call[None])[0]
        _check_alternatives(got, want, regions, m, case, call, 'model, event %s' % (event,))
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=4, num_chains=3, seed=4)
    ps = synthetic.make_init_params(e, 4, 4)
    regions = [(0, 5), (12, 30), (39, 39)]
    event = (None, 'total')

    def against_twin(models, batch_of, got, cns, tag):
        for r, mod in enumerate(models):
            c = Case(mod)
            st = posteriors.states_in_model_order(cns[r], batch_of(r), mod.seg_fwd_remap)
            want = posteriors.batch_region_alternatives(_twin_batch(c), 0, 1, regions, mod.seg_fwd_remap, mod.seg_is_original, mod.is_telomere,
                                                        k=3, event=event, cn=st[None])[0]
            _check_alternatives(got[r], want, regions, mod, c, st, '%s, restart %d' % (tag, r))

    rs = RestartSet(e, ps[:2], 4, num_clones=3, quiet=True, seeds=[0, 1])
    try:
        rs.variational_update(2)
        cns = [x['cn'] for x in rs.results()]
        against_twin(rs.models, lambda r: rs.batch, rs.region_alternatives(regions, 3, event, cns), cns, 'set')
        dec = rs.region_alternatives(regions, 3, event)
        assert all(np.array_equal(a['log_prob'], c['log_prob']) for x, y in zip(dec, rs.region_alternatives(regions, 3, event, cns)) for a, c in zip(x, y))
    finally:
        rs.close()
    groups = RestartGroups(e, ps, 4, groups=2, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    try:
        groups.variational_update(2)
        cns = [x['cn'] for x in groups.results()]
        got = groups.region_alternatives(regions, 3, event, cns)
        assert len(got) == 4
        against_twin(groups.models, lambda r: groups.models[r].model._batch, got, cns, 'groups')
    finally:
        groups.close()
    dg = DatasetGroups([e, e], [ps[:2], ps[2:4]], 4, seeds=[[0, 1], [2, 3]], num_clones=3, quiet=True)
    try:
        dg.variational_update(1)
        res = dg.results_by_dataset()
        cns = [[x['cn'] for x in part] for part in res]
        got = dg.region_alternatives(regions, 3, event, cns)
        assert len(got) == 2 and all(len(part) == 2 for part in got)
        for d, part in enumerate(dg.parts):
            against_twin(part.models, lambda r, part=part: part.models[r].model._batch, got[d], cns[d], 'dataset %d' % d)
    finally:
        dg.close()
