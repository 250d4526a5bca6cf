"""Locus joints on the device (rmx_locus_joint / k_locus_joint): against the log-domain numpy twin on the read-back
framelogprob / log_transmat -- in probability and, because every column has its own scale, in the log domain --, the
identities that tie a table to posterior_marginals and to rmx_region_pattern, bit-identity of the profile form, of restart
ranges, batches, nrow and staging chunks, two state classes, the mixed transition model, inserted segments, the sampler, no
side effects on the model, errors, and the public forms at the four class levels.

A crafted zero normaliser is left out: the siblings' tests show no way to make D(s') zero under positive mass that does not
go through set_array on the forward plane of a live batch, which none of them does."""
import ctypes as C

import numpy as np
import pytest

from remixt_amd import posteriors, restarts, synthetic
from tests import helpers as H
from tests import locus_twin
from tests.test_hip_region_events import Case
from tests.test_hip_sample_cn import GRIDS, _fitted, _model_state

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (5, 16), (16, 5), (16, 16))
# (row table, column table): the same total; clone 1's total against clone 2's major copy number; a mask table against a total
SPECS = [('peak_total_any', 'peak_total_any'), ('peak_total_1', 'peak_major_2'), ('loh', 'peak_total_any')]


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


def _lse(v, axis):
    with np.errstate(divide='ignore', invalid='ignore'):
        m = np.max(v, axis=axis, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.)
        return np.squeeze(m, axis) + np.log(np.exp(v - m).sum(axis=axis))


class LocusCase(Case):
    def __init__(self, *args, **kw):
        Case.__init__(self, *args, **kw)
        self._twin_tables = {}

    def tables(self, bins=16, first_level=0):
        levels, names = posteriors.locus_level_tables(self.b.cn_classes, bins, first_level)
        return levels, names, dict((k, levels[self.b.seg_class, i]) for i, k in enumerate(names))

    def joint(self, pairs, nrow, ncol, specs=SPECS, nslot=0, r0=None, nr=1, bins=16, first_level=0):
        levels, names, _ = self.tables(bins, first_level)
        q = np.array([[a, t, names.index(vr), names.index(vc)] for (a, t) in pairs for (vr, vc) in specs], dtype=np.int32)
        out = self.b.locus_joint_raw(self.r if r0 is None else r0, nr, q, levels, nrow, ncol, nslot)
        return out.reshape((nr, len(pairs), len(specs)) + out.shape[2:])

    def want(self, a, t, vr, vc, bins=16, first_level=0):
        """The twin's 16 x 16 table, computed once: a cell does not depend on the table's size."""
        key = (a, t, vr, vc, bins, first_level)
        if key not in self._twin_tables:
            _, _, lev_seg = self.tables(bins, first_level)
            self._twin_tables[key] = locus_twin.logtable(self.twin, a, t, 16, 16, lev_seg[vr], lev_seg[vc])
        return self._twin_tables[key]

    def check(self, pairs, sizes=SIZES, specs=SPECS, bins=16, first_level=0, tag=''):
        """|e^F - e^twin| <= L 1e-9 in every cell; |F - twin| <= L 1e-9 where the twin is >= -300; twin -inf -> -inf exactly; -inf
        -> the twin -inf, below -700, or more than 700 below its column's total.  Returns (worst error over bound, finite cells
        of the twin below -20 and above -300 in the 16 x 16 tables)."""
        worst, deep = 0., 0
        for nrow, ncol in sizes:
            got = self.joint(pairs, nrow, ncol, specs, bins=bins, first_level=first_level)[0]
            for i, (a, t) in enumerate(pairs):
                L = t - a + 1
                for j, (vr, vc) in enumerate(specs):
                    full = self.want(a, t, vr, vc, bins, first_level)
                    want, g = full[:nrow, :ncol], got[i, j]
                    assert g.shape == (nrow, ncol) and not np.isnan(g).any(), (tag, nrow, ncol, a, t, vr, vc, g)
                    err = np.abs(np.exp(g) - np.exp(want))
                    loud = want >= -300
                    with np.errstate(invalid='ignore'):
                        lerr = np.where(loud, np.abs(g - want), 0.)
                    n_deep = int(((want > -300) & (want < -20)).sum()) if (nrow, ncol) == (16, 16) else 0
                    deep += n_deep
                    worst = max(worst, err.max() / (L * 1e-9), lerr.max() / (L * 1e-9))
                    print('%s %d x %d pair (%d, %d) rows %s columns %s: max |P - twin| %.3e, max |F - twin| (twin >= -300) %.3e, %d cells in (-300, -20), lowest finite twin %.1f' % (
                        tag, nrow, ncol, a, t, vr, vc, err.max(), lerr.max(), n_deep, want[np.isfinite(want)].min() if np.isfinite(want).any() else np.nan))
                    assert (err <= L * 1e-9).all(), (tag, nrow, ncol, a, t, vr, vc, g, want)
                    assert (lerr <= L * 1e-9).all(), (tag, nrow, ncol, a, t, vr, vc, g, want)
                    assert (g[want == -np.inf] == -np.inf).all(), (tag, nrow, ncol, a, t, vr, vc, g, want)
                    column_total = np.broadcast_to(_lse(full[:, :ncol], 0)[None, :], want.shape)      # (over every row of the twin's column)
                    lost = g == -np.inf
                    assert ((want[lost] < -700) | (want[lost] < column_total[lost] - 700)).all(), (tag, nrow, ncol, a, t, vr, vc, g, want)
        print('%s worst error over bound: %.3e; cells in (-300, -20): %d' % (tag, worst, deep))
        return worst, deep


def _close(*models):
    """The device batches of fitted models, given back now and not whenever the collector finds them."""
    for m in models:
        m.model._batch.close()


@pytest.fixture(scope='module')
def cases(hip):
    made = dict(((N, M, c), LocusCase(_fitted(hip, N, M, c))) for N, M, c in GRIDS)
    yield made
    _close(*[case.m for case in made.values()])


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_twin(hip, cases, N, M, max_cn):
    """Case.queries() as pairs: a = t, neighbours over a plain and over a breakend adjacency, the ends of the longest chain, a
    chain start and a chain end.  The log-domain case that is not vacuous: the ends of the longest chain with the tumour
    clones' highest total on both sides, where the twin alone shows finite cells below -20."""
    case = cases[(N, M, max_cn)]
    assert case.S == {8: 165, 12: 355, 6: 457}[max_cn] and case.S % 16
    assert case.m.num_breakpoints > 0 and (case.bidx >= 0).any()
    pairs = case.queries()
    assert any(a == t for a, t in pairs) and any(case.bidx[a] >= 0 and t == a + 1 for a, t in pairs)
    worst, _ = case.check(pairs, tag='S %d' % case.S)
    assert worst <= 1.
    c = int(np.argmax(case.ce - case.cs))
    ends = (int(case.cs[c]), int(case.ce[c]))
    assert ends in pairs
    twin_alone = case.want(ends[0], ends[1], 'peak_total_any', 'peak_total_any')
    assert ((twin_alone > -300) & (twin_alone < -20)).sum() >= 1, twin_alone
    _, deep = case.check([ends], sizes=((16, 16),), specs=SPECS[:1], tag='S %d chain ends' % case.S)
    assert deep >= 1
    # a window that starts above 0: first_level 2, six bins
    worst, _ = case.check(pairs[1:5], sizes=((6, 6),), specs=[('peak_total_1', 'peak_total_any')], bins=6, first_level=2, tag='S %d first_level 2' % case.S)
    assert worst <= 1.
    # the model-level form
    levels, names, _ = case.tables()
    q = np.array([[a, t, 0, 3] for a, t in pairs], dtype=np.int32)
    one = case.m.model.locus_joint(q, levels, 5, 7)
    assert one.shape == (len(q), 5, 7) and np.array_equal(one, case.b.locus_joint_raw(case.r, 1, q, levels, 5, 7)[0])
    prof = case.m.model.locus_joint(q[:2], levels, 5, 7, nslot=3)
    assert prof.shape == (2, 3, 5, 7)


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_identities(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    b, S = case.b, case.S
    levels, names, lev_seg = case.tables()
    assert levels.max() <= 15                                  # the tables cover every state at 16 x 16
    post = b.get_array(case.r, 'posterior_marginals')
    c = int(np.argmax(case.ce - case.cs))
    seg = np.arange(case.cs[c], case.ce[c] + 1)
    pairs = [(int(a), int(t)) for a in seg[::2] for t in seg if a <= t]
    L = np.array([t - a + 1 for a, t in pairs])
    got = case.joint(pairs, 16, 16)[0]
    assert not np.isnan(got).any()

    def level_marginal(n, v):
        return np.array([post[n][lev_seg[v][n] == k].sum() for k in range(16)])
    worst = 0.
    for j, (vr, vc) in enumerate(SPECS):
        P = np.exp(got[:, j])
        ma = np.array([level_marginal(a, vr) for a, _ in pairs]); mt = np.array([level_marginal(t, vc) for _, t in pairs])
        # (i) the sums over rows and over columns are the level marginals of t and of a; the whole table sums to 1
        e1, e2, e3 = np.abs(P.sum(axis=1) - mt).max(axis=1), np.abs(P.sum(axis=2) - ma).max(axis=1), np.abs(P.sum(axis=(1, 2)) - 1)
        worst = max(worst, (np.maximum(np.maximum(e1, e2), e3) / L).max())
        assert (e1 <= L * 1e-9).all() and (e2 <= L * 1e-9).all() and (e3 <= L * 1e-9).all(), (vr, vc, e1.max(), e2.max(), e3.max())
        # (ii) mutual information is >= 0 and at most the smaller marginal entropy
        s = posteriors.joint_summary(got[:, j])
        Hm = lambda p: -np.where(p > 0, p * np.log(np.where(p > 0, p, 1.)), 0.).sum(axis=-1)
        assert (s['mutual_information'] >= 0).all() and (s['mutual_information'] <= np.minimum(Hm(s['marginal_a']), Hm(s['marginal_b'])) + L * 1e-8).all()
    print('S %d: marginal identities, worst error / L: %.3e over %d pairs' % (S, worst, len(pairs)))
    # (iii) a = t is the direct sum of post_t over the states that carry both levels
    own = case.joint([(int(n), int(n)) for n in range(case.N)], 16, 16)[0]
    for j, (vr, vc) in enumerate(SPECS):
        for n in range(case.N):
            want = np.zeros((16, 16))
            np.add.at(want, (lev_seg[vr][n], lev_seg[vc][n]), post[n])
            assert np.abs(np.exp(own[n, j]) - want).max() <= 1e-12, (vr, vc, n)
            assert (own[n, j][want == 0] == -np.inf).all() and (want[own[n, j] == -np.inf] < 1e-300).all(), (vr, vc, n)
    # (iv) every cell against rmx_region_pattern with 0/1 masks on one-segment pieces
    sub = [p for p in pairs if p[0] < p[1]][::3]
    Ls = np.array([t - a + 1 for a, t in sub])
    for vr, vc in SPECS:
        g = case.joint(sub, 16, 16, [(vr, vc)])[0, :, 0]
        masks = np.concatenate([levels[:, names.index(vr), None, :] == np.arange(16)[None, :, None],
                                levels[:, names.index(vc), None, :] == np.arange(16)[None, :, None]], axis=1).astype(np.uint8)
        pieces = np.array([[x, x, k, -1] for a, t in sub for i in range(16) for j in range(16) for x, k in ((a, i), (t, 16 + j))], dtype=np.int32)
        qq = np.array([[2 * k, 2, 0, 0] for k in range(len(sub) * 256)], dtype=np.int32)
        ref = b.region_pattern_raw(case.r, 1, qq, pieces, masks, None, None)[0].reshape(len(sub), 16, 16)
        err = np.abs(np.exp(g) - np.exp(ref))
        print('S %d: rows %s columns %s against 256 pattern queries per pair: max |dP| %.3e' % (S, vr, vc, err.max()))
        assert (err <= Ls[:, None, None] * 1e-9).all(), (vr, vc)
        assert (g[ref == -np.inf] == -np.inf).all()
        lost = (g == -np.inf) & (ref > -np.inf)
        total = np.broadcast_to(_lse(ref, 1)[:, None, :], ref.shape)
        assert ((ref[lost] < -700) | (ref[lost] < total[lost] - 700)).all(), (vr, vc)


def test_bit_identity(hip, cases):
    """A cell depends on neither nslot, nrow, the batch of queries nor their order."""
    case = cases[GRIDS[0]]
    c = int(np.argmax(case.ce - case.cs))
    a, t = int(case.cs[c]), int(case.ce[c])
    L = t - a + 1
    pairs = [(n, t) for n in range(t, a - 1, -1)]
    pair_form = case.joint(pairs, 16, 16)[0]                                  # (L, specs, 16, 16): the table of (t - k, t)
    for nslot in (L, L + 3):
        prof = case.joint([(a, t)], 16, 16, nslot=nslot)[0, 0]              # (specs, nslot, 16, 16)
        assert prof.shape == (len(SPECS), nslot, 16, 16)
        assert np.array_equal(np.moveaxis(prof[:, :L], 1, 0), pair_form) and np.isnan(prof[:, L:]).all()
    # a shorter query of the same profile call, and a = t in the profile form
    prof = case.joint([(t - 2, t), (t, t), (a, t)], 16, 16, nslot=L)[0]
    assert np.array_equal(np.moveaxis(prof[0][:, :3], 1, 0), pair_form[:3]) and np.isnan(prof[0][:, 3:]).all()
    assert np.array_equal(prof[1][:, 0], pair_form[0]) and np.isnan(prof[1][:, 1:]).all()
    # any nrow >= i + 1 for the cells it contains (columns select states: they are another walk)
    for nrow in (1, 5, 9):
        assert np.array_equal(case.joint(pairs, nrow, 16)[0], pair_form[..., :nrow, :]), nrow
    assert np.array_equal(case.joint([(a, t)], 5, 16, nslot=L)[0, 0, :, :L], np.moveaxis(pair_form[..., :5, :], 0, 1))
    # any batch and order of queries
    every = case.queries()
    full = case.joint(every, 16, 16)[0]
    for i in range(len(every)):
        assert np.array_equal(case.joint(every[i:i + 1], 16, 16)[0, 0], full[i]), i
    assert np.array_equal(case.joint(every[::-1], 16, 16)[0], full[::-1])
    assert np.array_equal(case.joint(every, 16, 16, SPECS[::-1])[0], full[:, ::-1])


def test_restart_ranges_and_mixed_transition_model(hip):
    """Four restarts; then restarts 1 and 2 take their snapshot under transition model 1: a call over 0 .. 3 has three launches
    and equals the single-restart calls bit for bit; restarts 0 and 1 agree with the twin on their own snapshot."""
    from tests.test_hip_query_driver import _restart_set
    rs = _restart_set(4)
    try:
        b = rs.batch
        case = LocusCase(rs.models[0])
        pairs = case.queries()
        call = lambda r0, nr, nslot=0: case.joint(pairs, 16, 16, r0=r0, nr=nr, nslot=nslot)
        for mixed in (False, True):
            if mixed:
                b.transition_model = 1
                b.update_p_cn(1, 3)
            full = call(0, 4)
            assert full.shape == (4, len(pairs), len(SPECS), 16, 16) and not np.isnan(full).any()
            assert len(np.unique(full.reshape(4, -1), axis=0)) > 1
            for r in range(4):
                assert np.array_equal(call(r, 1)[0], full[r]), (mixed, r)
            assert np.array_equal(call(1, 2), full[1:3]) and np.array_equal(call(1, 3), full[1:])
            longest = max(t - a + 1 for a, t in pairs)
            prof = call(0, 4, longest)
            for i, (a, t) in enumerate(pairs):
                assert np.array_equal(prof[:, i, :, t - a], full[:, i]), (mixed, i)
        for c in [LocusCase(rs.models[r]) for r in (0, 1)]:
            worst, _ = c.check(pairs, sizes=((16, 16),), tag='mixed model, restart %d' % c.r)
            assert worst <= 1.
    finally:
        rs.close()


def test_two_staging_chunks(hip, cases):
    """Nine short profile queries of one restart with 4096 slots of 16 x 16: 8 MiB each, so that the 64 MiB staging buffer holds
    seven of them and the call runs in two chunks."""
    case = cases[GRIDS[0]]
    levels, names, _ = case.tables()
    assert (64 << 20) // (4096 * 256 * 8 + 16) == 7
    c = int(np.argmax(case.ce - case.cs))
    t = int(case.ce[c])
    q = np.array([[t - k % 3, t, 3, k % 4] for k in range(9)], dtype=np.int32)
    big = case.b.locus_joint_raw(case.r, 1, q, levels, 16, 16, 4096)[0]
    small = case.b.locus_joint_raw(case.r, 1, q, levels, 16, 16, 3)[0]
    assert big.shape == (9, 4096, 16, 16) and np.array_equal(big[:, :3], small, equal_nan=True) and np.isnan(big[:, 3:]).all()
    assert not np.isnan(small[:, 0]).any() and np.isnan(small[0, 1:]).all() and not np.isnan(small[2]).any()


def test_two_classes(hip):
    m, h, e = H.make_model(hip, N=40, M=3, max_cn=4, chains=3)
    M = 3
    classes, _ = m._state_tables(M)
    classes = np.repeat(classes[:1], 2, axis=0)
    classes[1, :, 1, :] += 1                                             # class 1: clone 1 has one more copy of each allele
    N = m.N1
    seg_class = (np.arange(N) % 2).astype(np.int32)                      # 0, 1, 0, 1, ...
    brk_states = m.create_brk_states(M, m.max_copy_number, m.max_copy_number_diff)
    b = hip.RemixtBatch(M, N, m.num_breakpoints, m.normal_contamination, classes, seg_class, brk_states, np.asarray(h, dtype=float)[None],
                        m.l1, m.x1[:, 2].copy(), m.x1[:, 0:2].copy(), m.is_telomere, m.breakpoint_idx, m.breakpoint_orient,
                        m.transition_log_prob, [m.divergence_weight])
    try:
        b.set_array(0, 'allele_likelihood_mask', np.zeros(N, dtype=np.int64))
        b.variational_update(2)
        case = LocusCase(m, batch=b, r=0)
        levels, names, _ = case.tables()
        i = names.index('peak_total_1')
        assert np.array_equal(levels[1, i], levels[0, i] + 2)             # the level differs per class
        worst, _ = case.check(case.queries(), sizes=((16, 16),), tag='two classes')
        assert worst <= 1.
        # (a kernel that took class 0's levels everywhere would find clone 1 at total 0 or 1 in the odd segments)
        odd = case.joint([(n - 1, n) for n in range(1, N, 2) if case.tel[n - 1] == 0], 16, 16, [('peak_total_1', 'peak_total_1')])[0, :, 0]
        assert (odd[:, :, :2] == -np.inf).all() and np.isfinite(odd[:, :, 2:]).any()
    finally:
        b.close()


def _inserted(hip):
    e = synthetic.make_experiment(60, num_clones=3, max_copy_number=4, num_chains=3, seed=7)
    e.breakpoints = H.add_shared_boundary_breakpoints(e)
    m, h, _ = H.make_model(hip, M=3, max_cn=4, experiment=e)
    H.attach(m, h)
    m.model.allele_likelihood_mask = np.zeros(m.model.num_segments, dtype=int)      # (events of intermediate probability)
    m.variational_update(); m.variational_update()
    return m


def test_inserted_segments(hip):
    """Two breakends on one boundary: the model inserts a zero-length segment there.  The walk passes through it like through
    any other segment, and the dependence profile drops its slot."""
    m = _inserted(hip)
    case = LocusCase(m)
    assert m.N1 > m.N and not case.constrain.all()
    dummy = int(np.flatnonzero(~case.constrain & (np.arange(m.N1) > 0) & (case.tel == 0))[0])
    assert case.constrain[dummy - 1] and case.constrain[dummy + 1]
    pairs = [(dummy - 1, dummy + 1), (dummy, dummy), (dummy, dummy + 1), (dummy - 3, dummy + 2)]
    worst, _ = case.check(pairs, sizes=((16, 16),), tag='inserted segment')
    assert worst <= 1.
    # the experiment pair around it, through locus_joint and through the profile of locus_dependence
    i = int(m.seg_rev_remap[dummy - 1])
    assert m.seg_fwd_remap[i] == dummy - 1 and m.seg_fwd_remap[i + 1] == dummy + 1
    out = m.locus_joint([(i, i + 1), (i + 1, i)], feature=('total', 1), other='loh', bins=6)
    levels, names, lev_seg = case.tables(6)
    want = locus_twin.logtable(case.twin, dummy - 1, dummy + 1, 6, 6, lev_seg['peak_total_1'], lev_seg['loh'])
    assert np.abs(out['joint'][0] - np.exp(want)).max() <= 3e-9
    want = locus_twin.logtable(case.twin, dummy - 1, dummy + 1, 6, 6, lev_seg['loh'], lev_seg['peak_total_1'])
    assert np.abs(out['joint'][1] - np.exp(want).T).max() <= 3e-9
    dep = m.locus_dependence([i + 1, i], window=2, feature=('total', 1), other='loh', bins=6)
    assert dep['segment'][0, 1] == i and dep['segment'][0, 2] == i + 1
    ref = m.locus_joint([(i + 1, i), (i, i + 1)], feature=('total', 1), other='loh', bins=6)
    for k in posteriors.DEPENDENCE_ARRAYS:
        assert np.array_equal(dep[k][0, 1], ref[k][0], equal_nan=True) and np.array_equal(dep[k][1, 3], ref[k][1], equal_nan=True), k
    _close(m)


def test_against_the_sampler(hip):
    """The tables of the masked case of test_hip_region_events.test_against_the_sampler against 4 096 posterior samples (seed
    99): every cell within 5 sqrt(p (1 - p) / 4096) + 1 / 4096."""
    from tests.test_hip_posterior_summary import _fitted as fitted_masked
    m = fitted_masked(hip, 30, 3, 8, sweeps=3, masked=True)
    NS, K = 4096, 10
    b, r = m.model._batch, m.model._r
    st = b.sample_states(r, 1, NS, [99]).astype(np.int64)[0]                      # (NS, N1)
    levels, names = posteriors.locus_level_tables(b.cn_classes, K)
    fwd = np.asarray(m.seg_fwd_remap)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    chain = np.searchsorted(ce, fwd, side='left')
    pairs = [(i, j) for i, j in ((0, 0), (3, 4), (11, 2), (0, 9), (12, 29), (5, 6), (20, 14)) if chain[i] == chain[j]]
    assert len(pairs) >= 4
    informative = 0
    for feature, other in ((('total', 'any'), None), (('total', 1), ('major', 2)), ('loh', ('total', 'any'))):
        out = m.locus_joint(pairs, feature=feature, other=other, bins=K)
        fi = names.index(posteriors.locus_feature_name(feature, 3))
        oi = fi if other is None else names.index(posteriors.locus_feature_name(other, 3))
        for k, (i, j) in enumerate(pairs):
            li = levels[b.seg_class[fwd[i]], fi][st[:, fwd[i]]]
            lj = levels[b.seg_class[fwd[j]], oi][st[:, fwd[j]]]
            freq = np.bincount(li * K + lj, minlength=K * K).reshape(K, K) / NS
            P = out['joint'][k]
            tol = 5 * np.sqrt(P * (1 - P) / NS) + 1. / NS
            informative += int(((P > 0.01) & (P < 0.99)).sum())
            assert (np.abs(freq - P) <= tol).all(), (feature, other, i, j, freq, P)
    print('informative (pair, cell) entries: %d' % informative)
    assert informative >= 3
    _close(m)


def test_no_side_effects(hip):
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    before = _model_state(m1)
    out = m1.locus_joint([(0, 10), (5, 5), (12, 3)], bins=16)
    dep = m1.locus_dependence([7, 30], window=5)
    assert out['joint'].shape == (3, 16, 16) and out['bins'] == 16 and dep['p_equal'].shape == (2, 11)
    after = _model_state(m1)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    for m in (m1, m2):
        m.variational_update()
    s1, s2 = _model_state(m1), _model_state(m2)
    for k in s1:
        assert np.array_equal(s1[k], s2[k], equal_nan=True), k
    assert m1.model.calculate_elbo() == m2.model.calculate_elbo()
    _close(m1, m2)


def test_errors(hip):
    from remixt_amd import bpmodel
    m, h, e = H.make_model(hip, N=30, M=3, max_cn=3)
    H.attach(m, h)
    b, r = m.model._batch, m.model._r
    levels, names = posteriors.locus_level_tables(b.cn_classes, 4)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    ok = [[int(cs[0]), int(cs[0]) + 1, 0, 1]]
    with pytest.raises(ValueError, match='update_p_cn'):
        b.locus_joint_raw(r, 1, ok, levels, 4, 4)
    assert bpmodel.last_error_restarts() == [r]
    with pytest.raises(ValueError, match='update_p_cn'):
        m.locus_joint([(0, 3)])
    m.variational_update()
    N, T = b.num_segments, len(names)
    lib, handle = b._lib, b._handle
    dp = C.POINTER(C.c_double)
    assert b.locus_joint_raw(r, 1, ok, levels, 4, 4).shape == (1, 1, 4, 4) and b.locus_joint_raw(r, 1, ok, levels, 4, 4, 2).shape == (1, 1, 2, 4, 4)
    negative = levels.copy(); negative[-1, -1, -1] = -1
    # (queries, nrow, ncol, nslot, levels, words of the message)
    bad = [(ok, 0, 4, 0, levels, 'rows and of columns'), (ok, 17, 4, 0, levels, 'rows and of columns'), (ok, 4, 0, 0, levels, 'rows and of columns'),
           (ok, 4, 17, 0, levels, 'rows and of columns'), (ok, 4, -1, 2, levels, 'rows and of columns'), (ok, 4, 4, -1, levels, 'nslot'), (ok, 4, 4, 4097, levels, 'nslot'),
           (ok + [[0, 1, -1, 0]], 4, 4, 0, levels, 'row level index'), (ok + [[0, 1, T, 0]], 4, 4, 0, levels, 'row level index'),
           (ok + [[0, 1, 0, -1]], 4, 4, 0, levels, 'column level index'), (ok + [[0, 1, 0, T]], 4, 4, 0, levels, 'column level index'),
           (ok, 4, 4, 0, negative, 'level entry is negative'), (ok + [[3, 2, 0, 0]], 4, 4, 0, levels, 'first <= last'),
           (ok + [[int(ce[0]), int(ce[0]) + 1, 0, 0]], 4, 4, 0, levels, 'chain end'), (ok + [[int(cs[0]), int(ce[1]), 0, 0]], 4, 4, 3, levels, 'chain end'),
           (ok + [[0, N, 0, 0]], 4, 4, 0, levels, 'first <= last'), (ok + [[-1, 0, 0, 0]], 4, 4, 0, levels, 'first <= last'),
           (ok + [[int(cs[0]), int(cs[0]) + 2, 0, 0]], 4, 4, 2, levels, 'longer than nslot'), (ok, 4, 4, 1, levels, 'longer than nslot')]
    for q, nrow, ncol, nslot, lv, text in bad:
        # through the C entry point with an output buffer of its own: refused, and the buffer is untouched
        qa, args, _keep = b._region_args(q, None, lv, None)
        obuf = np.full((len(q), 8, 16, 16), 7.25)
        rc = lib.rmx_locus_joint(handle, r, 1, args[0], args[1], args[4], args[5], nrow, ncol, nslot, obuf.ctypes.data_as(dp))
        assert rc == 5 and (obuf == 7.25).all(), (q, nrow, ncol, nslot, text, rc)
        with pytest.raises(ValueError, match='^bad argument: .*' + text):
            b.locus_joint_raw(r, 1, q, lv, nrow, ncol, nslot)
        assert bpmodel.last_error_restarts() == []
    qa, args, _keep = b._region_args(ok, None, levels, None)
    obuf = np.full((2, 1, 4, 4), 7.25)
    out = obuf.ctypes.data_as(dp)
    for r0, nr in ((-1, 1), (0, 0), (0, 2)):
        assert lib.rmx_locus_joint(handle, r0, nr, args[0], args[1], args[4], args[5], 4, 4, 0, out) == 5
    # nq < 1, NULL pointers, nlevel < 1
    assert lib.rmx_locus_joint(handle, r, 1, 0, args[1], args[4], args[5], 4, 4, 0, out) == 5
    assert lib.rmx_locus_joint(handle, r, 1, args[0], None, args[4], args[5], 4, 4, 0, out) == 5
    assert lib.rmx_locus_joint(handle, r, 1, args[0], args[1], args[4], None, 4, 4, 0, out) == 5
    assert lib.rmx_locus_joint(handle, r, 1, args[0], args[1], 0, args[5], 4, 4, 0, out) == 5
    assert lib.rmx_locus_joint(handle, r, 1, args[0], args[1], args[4], args[5], 4, 4, 0, None) == 5
    assert (obuf == 7.25).all()
    assert lib.rmx_locus_joint(handle, r, 1, args[0], args[1], args[4], args[5], 4, 4, 0, out) == 0 and not (obuf[0] == 7.25).any() and (obuf[1] == 7.25).all()
    for kw in (dict(bins=17), dict(feature=('total', 3)), dict(feature=('depth', 1)), dict(other='gain')):
        with pytest.raises(ValueError):
            m.locus_joint([(0, 3)], **kw)
    with pytest.raises(ValueError):
        m.locus_dependence([30])
    from oracle import oracle
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError):
        mo.locus_joint([(0, 3)])
    _close(m)


PAIRS = [(2, 7), (7, 2), (17, 17), (10, 30), (39, 0), (12, 13)]
EXAMPLES = {'locus_joint': [dict(pairs=PAIRS), dict(pairs=PAIRS, feature=('major', 'any'), other='loh', bins=5, first_level=1)],
            'locus_dependence': [dict(anchors=[3, 17, 39], window=4), dict(anchors=[12], window=9, feature='loh', other=('total', 2), bins=6)]}
SHARED = {'locus_joint': ('bins', 'first_level'), 'locus_dependence': ('bins', 'first_level', 'segment')}


def _direct(name, b, r0, nr, m, a):
    maps = (m.seg_fwd_remap, m.seg_is_original, m.is_telomere)
    if name == 'locus_joint':
        return posteriors.batch_locus_joint(b, r0, nr, a['pairs'], *maps, feature=a.get('feature', ('total', 1)), other=a.get('other'), bins=a.get('bins', 8),
                                            first_level=a.get('first_level', 0))
    return posteriors.batch_locus_dependence(b, r0, nr, a['anchors'], *maps, window=a.get('window', 32), feature=a.get('feature', ('total', 1)), other=a.get('other'),
                                             bins=a.get('bins', 8), first_level=a.get('first_level', 0))


def _same(a, b, where):
    assert isinstance(a, dict) and isinstance(b, dict) and list(a) == list(b), where
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == 'f'), (where, k)


def test_the_four_class_levels(hip):
    """Every level returns the numbers of posteriors.batch_locus_joint / batch_locus_dependence called directly; the
    dependence profile of an anchor equals locus_joint on the pairs it stands for."""
    from remixt_amd import queries
    R, MAX_CN = 4, 4
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=MAX_CN, num_chains=3, seed=4)
    ps = synthetic.make_init_params(e, R, MAX_CN)
    rs = restarts.RestartSet(e, ps, MAX_CN, num_clones=3, quiet=True, seeds=list(range(R)), options={'fb_nv': 1})
    try:
        rs.variational_update(2)
        b, models = rs.batch, rs.models
        cs, ce = posteriors.chains_from_telomeres(models[0].is_telomere)
        chain = np.searchsorted(ce, models[0].seg_fwd_remap, side='left')
        assert chain[2] == chain[7] and chain[10] != chain[30] and chain[0] != chain[39]
        set_answers = {}
        for name, examples in EXAMPLES.items():
            for k, given in enumerate(examples):
                want = _direct(name, b, 0, R, models[0], given)
                got = getattr(rs, name)(**given)
                _same(got, want, 'set: %s %r' % (name, given))
                set_answers[(name, k)] = got
                for r, m in enumerate(models):
                    one = _direct(name, b, r, 1, m, given)
                    one = dict((key, v if key in SHARED[name] else v[0]) for key, v in one.items())
                    _same(getattr(m, name)(**given), one, 'model %d: %s %r' % (r, name, given))
        # a cross-chain pair is the product of its marginals: no information
        lj = set_answers[('locus_joint', 0)]
        assert (lj['mutual_information'][:, 3] <= 1e-12).all() and np.abs(lj['joint'].sum(axis=(-2, -1)) - 1).max() <= 1e-7
        assert np.array_equal(lj['log_joint'][:, 1], np.swapaxes(lj['log_joint'][:, 0], -1, -2))
        # locus_dependence of an anchor equals locus_joint on the pairs it stands for
        for k, given in enumerate(EXAMPLES['locus_dependence']):
            dep = set_answers[('locus_dependence', k)]
            at = [(i, j) for i in range(len(given['anchors'])) for j in range(dep['segment'].shape[1]) if dep['segment'][i, j] >= 0]
            pairs = [(given['anchors'][i], int(dep['segment'][i, j])) for i, j in at]
            assert len(pairs) > len(given['anchors']) and (dep['segment'][:, given['window']] == given['anchors']).all()
            ref = rs.locus_joint(pairs, **dict((key, v) for key, v in given.items() if key not in ('anchors', 'window')))
            for key in posteriors.DEPENDENCE_ARRAYS:
                got = np.stack([dep[key][:, i, j] for i, j in at], axis=1)
                assert np.array_equal(got, ref[key], equal_nan=True), (k, key)
                assert np.isnan(dep[key][:, dep['segment'] < 0]).all()
            assert np.abs(dep['p_equal'][:, :, given['window']] - 1).max() <= 1e-9 or given.get('other') is not None
    finally:
        rs.close()
    g = restarts.RestartGroups(e, ps, MAX_CN, groups=2, num_clones=3, quiet=True, seeds=list(range(R)), options={'fb_nv': 1})
    try:
        g.variational_update(2)
        g.synchronize()
        for name, examples in EXAMPLES.items():
            entry = queries.BY_NAME[name]
            for k, given in enumerate(examples):
                parts = [getattr(part, name)(**given) for part in g.sets]
                got = getattr(g, name)(**given)
                _same(got, restarts._join(parts, shared=entry.shared), 'groups: %s %r' % (name, given))
                assert got['p_equal'].shape == set_answers[(name, k)]['p_equal'].shape
    finally:
        g.close()
    dg = restarts.DatasetGroups([e, e], [ps[:2], ps[2:]], MAX_CN, seeds=[[0, 1], [2, 3]], num_clones=3, quiet=True, options={'fb_nv': 1})
    try:
        dg.variational_update(2)
        dg.synchronize()
        for name, examples in EXAMPLES.items():
            for given in examples:
                want = [getattr(part, name)(**given) for part in dg.parts]
                got = getattr(dg, name)(**given)
                assert len(got) == 2
                for d in range(2):
                    _same(got[d], want[d], 'datasets: %s %r' % (name, given))
    finally:
        dg.close()
