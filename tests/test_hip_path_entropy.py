"""Path entropy on the device (rmx_path_entropy / k_path_entropy, k_path_entropy_adj): against the log-domain numpy twin on the
read-back framelogprob / log_transmat (every adjacency and every segment of five grids, 4 to 617 states), identities on the
device alone (posterior_marginals, posterior_summary_raw, rmx_locus_joint's full adjacent joint), the sampler, bit-identity of
restart ranges and of segment windows that move an adjacency to another tile and another row of it, two state classes, the
mixed transition model in both directions, no side effects on the model, errors, and the public form at the four class levels.

The staging chunk of a call is rmxh::entropy_chunk(nr, n1 - n0, 64 MiB): at 16 bytes per (restart, segment) it is below the
range only beyond four million (restart, segment) pairs, which no fixture has.  The chunk rule is exercised on the host
(tests/test_entropy_host_cpu.py); a chunk is a segment window, and the windows are exercised here on the four restarts of the
40-segment restart set, the call over all segments on the 60-segment grid, the largest N the fixtures have.

A crafted zero normaliser is left out, as in the siblings' tests: there is no way to make D(s') zero under positive mass that
does not go through set_array on the forward plane of a live batch."""
import ctypes as C

import numpy as np
import pytest

from remixt_amd import posteriors, restarts, synthetic
from tests import entropy_twin
from tests import helpers as H
from tests.test_hip_region_events import Case
from tests.test_hip_sample_cn import GRIDS, _fitted, _model_state

pytestmark = pytest.mark.gpu

# the siblings' grids (165, 355, 457 states), more than 512 states (the widest instantiation) and at most 16 states
WIDE, SMALL = (16, 3, 16), (40, 2, 2)
ALL_GRIDS = list(GRIDS) + [WIDE, SMALL]
STATES = {GRIDS[0]: 165, GRIDS[1]: 355, GRIDS[2]: 457, WIDE: 617}


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


class EntropyCase(Case):
    """Case with the twin's two arrays (computed once, never changed) and the device's."""

    def __init__(self, *args, **kw):
        Case.__init__(self, *args, **kw)
        self.want_marg, self.want_step = entropy_twin.arrays(self.twin)
        self.want_marg.flags.writeable = False
        self.want_step.flags.writeable = False
        inner = np.ones(self.N, dtype=bool)
        inner[self.ce] = False
        self.plain = np.flatnonzero(inner & (self.bidx < 0))
        self.breakend = np.flatnonzero(inner & (self.bidx >= 0))

    def raw(self, n0=0, n1=None, r0=None, nr=1):
        return self.b.path_entropy_raw(self.r if r0 is None else r0, nr, n0, n1)

    def check(self, tag):
        """Every segment and adjacency within 1e-9 of the twin, every run of Case.queries() and the longest chain within L 1e-9.
        Returns the worst error over its bound."""
        marg, step = self.raw()
        assert marg.shape == step.shape == (1, self.N) and marg.dtype == step.dtype == np.float64
        marg, step = marg[0], step[0]
        assert not np.isnan(marg).any() and not np.isnan(step).any()
        em, es = np.abs(marg - self.want_marg).astype(float), np.abs(step - self.want_step).astype(float)
        print('%s: max |marg - twin| %.3e, max |step - twin| %.3e (largest marg %.4f, largest step %.4f)' % (tag, em.max(), es.max(), marg.max(), step.max()))
        worst = max(em.max(), es.max()) / 1e-9
        assert (em <= 1e-9).all() and (es <= 1e-9).all(), tag
        assert (step[self.ce] == 0).all() and not np.signbit(step[self.ce]).any()
        c = int(np.argmax(self.ce - self.cs))
        runs = self.queries() + [(int(self.cs[c]), int(self.ce[c]))]
        got = posteriors.entropy_runs(marg, step, runs, self.constrain)['path_entropy']
        for (a, z), h in zip(runs, got):
            want = entropy_twin.run_entropy(self.want_marg, self.want_step, a, z)
            L = z - a + 1
            print('%s run [%d, %d]: H %.12g (twin %.12g), error %.3e' % (tag, a, z, h, float(want), abs(h - float(want))))
            worst = max(worst, abs(h - float(want)) / (L * 1e-9))
            assert abs(h - float(want)) <= L * 1e-9, (tag, a, z, h, want)
        print('%s worst error over bound: %.3e' % (tag, worst))
        return worst


def _close(*models):
    for m in models:
        m.model._batch.close()


@pytest.fixture(scope='module')
def cases(hip):
    from tests.test_hip_posterior_summary import _fitted as fitted_masked
    made = dict(((N, M, c), EntropyCase(_fitted(hip, N, M, c))) for N, M, c in ALL_GRIDS[:-1])
    # the small grid with its read counts masked out: a posterior spread over its states, so that steps are far from 0
    made[SMALL] = EntropyCase(fitted_masked(hip, *SMALL, masked=True))
    yield made
    _close(*[case.m for case in made.values()])


@pytest.mark.parametrize('N,M,max_cn', ALL_GRIDS)
def test_against_twin(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    if (N, M, max_cn) == SMALL:
        assert case.S <= 16
    else:
        assert case.S == STATES[(N, M, max_cn)] and case.S % 16
    assert (case.S > 512) == ((N, M, max_cn) == WIDE)
    # plain and breakend adjacencies; one state class, so one transition class: more than one tile, and somewhere a last tile that is not full
    assert len(case.plain) and len(case.breakend) and len(np.unique(case.b.seg_class)) == 1
    assert any(len(c.plain) > 16 and len(c.plain) % 16 for c in cases.values())
    worst = case.check('S %d' % case.S)
    assert worst <= 1.
    # a tile with a single member: the window of one plain adjacency; and the window of one breakend adjacency
    full_m, full_s = case.raw()
    for n in (int(case.plain[0]), int(case.plain[-1]), int(case.breakend[0])):
        m1, s1 = case.raw(n, n + 1)
        assert m1.shape == (1, 1) and m1[0, 0] == full_m[0, n] and s1[0, 0] == full_s[0, n]
        assert abs(s1[0, 0] - float(case.want_step[n])) <= 1e-9
    # the model-level form
    one_m, one_s = case.m.model.path_entropy()
    assert np.array_equal(one_m, full_m[0]) and np.array_equal(one_s, full_s[0])
    one_m, one_s = case.m.model.path_entropy(2, 9)
    assert np.array_equal(one_m, full_m[0, 2:9]) and np.array_equal(one_s, full_s[0, 2:9])


def _xlogx_sum(p):
    p = np.asarray(p, dtype=np.longdouble)
    q = p[p > 0]
    return float(-(q * np.log(q)).sum())


@pytest.mark.parametrize('N,M,max_cn', ALL_GRIDS)
def test_identities(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    b, r = case.b, case.r
    marg, step = (a[0] for a in case.raw())
    post = b.get_array(r, 'posterior_marginals')
    want = np.array([_xlogx_sum(row) for row in post])
    print('S %d: max |marg + sum p log p| %.3e' % (case.S, np.abs(marg - want).max()))
    assert np.abs(marg - want).max() <= 1e-12 * max(1., np.log(case.S))
    stats = b.posterior_summary_raw(r, 1, want_argmax=False)[1][0]
    print('S %d: max |marg - posterior_summary entropy| %.3e' % (case.S, np.abs(marg - stats[:, 1]).max()))
    assert np.abs(marg - stats[:, 1]).max() <= 1e-12 * max(1., np.log(case.S))
    assert (step >= 0).all() and (marg >= 0).all() and (step <= marg + 1e-12).all()
    regions = [(0, len(case.m.seg_fwd_remap) - 1), (1, 5), (3, 3)]
    out = posteriors.batch_path_entropy(b, r, 1, regions, case.m.seg_fwd_remap, case.m.seg_is_original, case.m.is_telomere)
    L = np.array([z - a + 1 for a, z in regions])
    print('S %d: total correlation %s, path entropy %s, perplexity %s' % (case.S, out['total_correlation'][0], out['path_entropy'][0], out['perplexity'][0]))
    assert (out['total_correlation'][0] >= -L * 1e-12).all()
    assert abs(out['total_correlation'][0, 2]) <= 1e-12 and out['path_entropy'][0, 2] == marg[case.m.seg_fwd_remap[3]]


def test_step_against_the_adjacent_joint(hip, cases):
    """At most 16 states: rmx_locus_joint with the state index as the level gives the full joint of two neighbours;
    H(joint) - H(column marginal) is the step, on plain and on breakend adjacencies."""
    case = cases[SMALL]
    b, r, S = case.b, case.r, case.S
    step = case.raw()[1][0]
    levels = np.ascontiguousarray(np.broadcast_to(np.arange(S, dtype=np.int16), b.cn_classes.shape[:2])[:, None, :])
    adj = np.concatenate([case.plain, case.breakend])
    q = np.array([[n, n + 1, 0, 0] for n in adj], dtype=np.int32)
    joint = np.exp(b.locus_joint_raw(r, 1, q, levels, S, S)[0])
    worst = 0.
    for i, n in enumerate(adj):
        want = _xlogx_sum(joint[i]) - _xlogx_sum(joint[i].sum(axis=0))
        worst = max(worst, abs(step[n] - want))
        assert abs(step[n] - want) <= 1e-9, (n, step[n], want)
    # (the fixture: steps four orders above the tolerance on both kinds of adjacency, so the comparison is not one of zeros)
    assert step[case.plain].max() > 1e-5 and step[case.breakend].max() > 1e-5
    print('S %d: max |step - (H(joint) - H(column))| %.3e over %d plain and %d breakend adjacencies; largest step %.4f' % (
        S, worst, len(case.plain), len(case.breakend), step.max()))


def test_against_the_sampler(hip):
    """-mean log q of 4 096 sampled paths over a run against the exact entropy: within 5 sd / sqrt(K) + 1e-9."""
    from tests.test_hip_posterior_summary import _fitted as fitted_masked
    m = fitted_masked(hip, 30, 3, 8, sweeps=3, masked=True)
    try:
        K = 4096
        case = EntropyCase(m)
        b, r = case.b, case.r
        st = b.sample_states(r, 1, K, [99])                      # (1, K, N1)
        marg, step = (a[0] for a in case.raw())
        c = int(np.argmax(case.ce - case.cs))
        be = int(case.breakend[0])
        mid = int(case.plain[len(case.plain) // 2])
        runs = [(mid, mid + 1), (be, be + 1), (int(case.cs[c]), int(case.ce[c]))]
        er = posteriors.entropy_runs(marg, step, runs, case.constrain)
        informative = 0
        for i, (a, z) in enumerate(runs):
            q = np.array([[a, z, -1, k] for k in range(K)], dtype=np.int32)
            lq = b.call_logprob_raw(r, 1, st, q, None, case.constrain)[0]
            assert np.isfinite(lq).all()
            est, tol = -lq.mean(), 5 * lq.std(ddof=1) / np.sqrt(K) + 1e-9
            Hx, slack = er['path_entropy'][i], er['inserted_slack'][i]
            print('run [%d, %d]: H %.6f slack %.3e, sampled %.6f +- %.6f' % (a, z, Hx, slack, est, tol))
            informative += int(Hx > 0.05)
            if case.constrain[a:z + 1].all():
                assert slack == 0 and abs(est - Hx) <= tol, (a, z, est, Hx, tol)
            else:
                assert Hx - slack - tol <= est <= Hx + tol, (a, z, est, Hx, slack, tol)
        assert informative >= 2
    finally:
        _close(m)


def test_bit_identity(hip):
    """A (restart, adjacency) entry depends on neither the restart range nor the segment window: windows of 1, 15, 16 and 17
    segments at every offset move an adjacency through every row of a tile and between tiles; the whole against its halves."""
    from tests.test_hip_query_driver import _restart_set
    rs = _restart_set(4)
    try:
        b = rs.batch
        N = b.num_segments
        fm, fs = b.path_entropy_raw(0, 4)
        assert fm.shape == (4, N) and not np.isnan(fm).any() and not np.isnan(fs).any() and len(np.unique(fs, axis=0)) > 1 and fs.max() > 1e-9
        for r in range(4):
            m1, s1 = b.path_entropy_raw(r, 1)
            assert np.array_equal(m1[0], fm[r]) and np.array_equal(s1[0], fs[r]), r
        m2, s2 = b.path_entropy_raw(1, 2)
        assert np.array_equal(m2, fm[1:3]) and np.array_equal(s2, fs[1:3])
        for width in (1, 15, 16, 17):
            for n0 in range(0, N - width + 1):
                mw, sw = b.path_entropy_raw(0, 4, n0, n0 + width)
                assert np.array_equal(mw, fm[:, n0:n0 + width]) and np.array_equal(sw, fs[:, n0:n0 + width]), (width, n0)
        h = N // 2
        (ma, sa), (mb, sb) = b.path_entropy_raw(0, 4, 0, h), b.path_entropy_raw(0, 4, h, N)
        assert np.array_equal(np.concatenate([ma, mb], axis=1), fm) and np.array_equal(np.concatenate([sa, sb], axis=1), fs)
    finally:
        rs.close()


def test_two_classes(hip):
    m, h, e = H.make_model(hip, N=40, M=3, max_cn=4, chains=3)
    M = 3
    classes, _ = m._state_tables(M)
    classes = np.repeat(classes[:1], 2, axis=0)
    classes[1, :, 1, :] += 1                                             # class 1: clone 1 has one more copy of each allele
    N = m.N1
    seg_class = (np.arange(N) % 2).astype(np.int32)                      # 0, 1, 0, 1, ...: two transition classes that alternate
    brk_states = m.create_brk_states(M, m.max_copy_number, m.max_copy_number_diff)
    b = hip.RemixtBatch(M, N, m.num_breakpoints, m.normal_contamination, classes, seg_class, brk_states, np.asarray(h, dtype=float)[None],
                        m.l1, m.x1[:, 2].copy(), m.x1[:, 0:2].copy(), m.is_telomere, m.breakpoint_idx, m.breakpoint_orient,
                        m.transition_log_prob, [m.divergence_weight])
    try:
        # (every other segment without read counts: steps far from 0 next to peaked ones)
        b.set_array(0, 'allele_likelihood_mask', np.zeros(N, dtype=np.int64))
        b.set_array(0, 'total_likelihood_mask', (np.arange(N) % 4 < 2).astype(np.int64))
        b.variational_update(2)
        case = EntropyCase(m, batch=b, r=0)
        marg, step = (a[0] for a in case.raw())
        em, es = np.abs(marg - case.want_marg).astype(float).max(), np.abs(step - case.want_step).astype(float).max()
        print('two classes: max |marg - twin| %.3e, max |step - twin| %.3e, largest step %.4f' % (em, es, step.max()))
        assert em <= 1e-9 and es <= 1e-9 and step.max() > 1e-5
    finally:
        b.close()


def test_mixed_transition_model(hip):
    """The snapshot of the last update_p_cn under another transition_model than the current one, both directions."""
    m = _fitted(hip, 40, 3, 4, seed=3)
    T0 = np.array(m.model.log_transmat)
    same = EntropyCase(m).raw()
    m.model.transition_model = 1
    assert np.array_equal(np.array(m.model.log_transmat), T0)            # the snapshot stays the model-0 one
    case = EntropyCase(m)
    assert case.check('mixed model 0 -> 1') <= 1.
    # exp(Tval) in place of the Wf table: the same numbers to rounding, not to the bit
    assert np.abs(case.raw()[1] - same[1]).max() <= 1e-12
    m2 = _fitted(hip, 40, 3, 4, seed=3, transition_model=1)
    m2.model.transition_model = 0
    case2 = EntropyCase(m2)
    assert not np.array_equal(np.array(m2.model.log_transmat), T0)
    assert case2.check('mixed model 1 -> 0') <= 1.
    _close(m, m2)


def test_no_side_effects(hip):
    """Every array tools/query_bits.py reads of the other queries (four restarts, two of them under the other transition model)
    is the same before and after calls that overwrite the staging and the table buffer those queries share; a fit continued
    after a call equals one without it."""
    from tests.test_hip_region_kbest import _query_bits
    qb = _query_bits()
    rs = qb.open_scenario(*qb.GRIDS[0])
    try:
        b, m = rs.batch, rs.models[0]
        before, state = {}, _model_state(m)
        qb.collect(rs, before)
        own = [k for k in before if 'path_entropy' in k]
        assert len(own) == 2 and len(before) >= 36
        for n0, n1 in ((0, None), (3, 40), (17, 18)):
            marg, step = b.path_entropy_raw(0, qb.R, n0, n1)
            assert not np.isnan(marg).any() and not np.isnan(step).any()
        rs.path_entropy([(0, 9), (20, 22), (40, 49)])
        after = {}
        qb.collect(rs, after)
        assert sorted(before) == sorted(after)
        for k in before:
            assert before[k].dtype == after[k].dtype and np.array_equal(before[k], after[k], equal_nan=before[k].dtype.kind == 'f'), k
        again = _model_state(m)
        for k in state:
            assert np.array_equal(state[k], again[k], equal_nan=True), k
    finally:
        rs.close()
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    before = _model_state(m1)
    out = m1.path_entropy([(0, 10), (5, 5), (3, 12)])
    assert out['path_entropy'].shape == (3,) and out['segment_entropy'].shape == (m1.N,) and out['step_entropy'].shape == (m1.N - 1,)
    m1.model.path_entropy(3, 20)
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
    with pytest.raises(ValueError, match='update_p_cn'):
        b.path_entropy_raw(r, 1)
    assert bpmodel.last_error_restarts() == [r]
    with pytest.raises(ValueError, match='update_p_cn'):
        m.path_entropy()
    m.variational_update()
    N = b.num_segments
    lib, handle = b._lib, b._handle
    dp = C.POINTER(C.c_double)
    mbuf, sbuf = np.full((2, N), 7.25), np.full((2, N), 7.25)
    mp, sp = mbuf.ctypes.data_as(dp), sbuf.ctypes.data_as(dp)
    call = lambda r0=r, nr=1, n0=0, n1=N, a=mp, s=sp: lib.rmx_path_entropy(handle, r0, nr, n0, n1, a, s)
    for kw in (dict(r0=-1), dict(nr=0), dict(nr=2), dict(n0=-1), dict(n0=3, n1=3), dict(n0=4, n1=3), dict(n1=N + 1), dict(n0=N, n1=N + 1), dict(a=None, s=None)):
        assert call(**kw) == 5, kw
    assert (mbuf == 7.25).all() and (sbuf == 7.25).all()
    for kw, text in ((dict(r0=1), 'restart range'), (dict(n0=5, n1=5), 'n0 < n1'), (dict(n1=N + 1), 'n0 < n1')):
        with pytest.raises(ValueError, match='^bad argument: .*' + text):
            b.path_entropy_raw(kw.get('r0', r), 1, kw.get('n0', 0), kw.get('n1', N))
        assert bpmodel.last_error_restarts() == []
    # either output alone
    assert call(a=None) == 0 and (mbuf == 7.25).all() and not (sbuf[0] == 7.25).any() and (sbuf[1] == 7.25).all()
    assert call(s=None) == 0 and not (mbuf[0] == 7.25).any() and (mbuf[1] == 7.25).all()
    both = b.path_entropy_raw(r, 1)
    assert np.array_equal(both[0][0], mbuf[0]) and np.array_equal(both[1][0], sbuf[0])
    with pytest.raises(ValueError):
        m.path_entropy([(3, 2)])
    with pytest.raises(ValueError):
        m.path_entropy([(0, m.N)])
    _close(m)


REGIONS = [(2, 7), (17, 17), (10, 30), (0, 39), (12, 13)]


def _same(a, b, where):
    assert isinstance(a, dict) and isinstance(b, dict) and list(a) == list(b), where
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), (where, k)


def test_the_four_class_levels(hip):
    """Every level returns the numbers of posteriors.batch_path_entropy called directly, which asks the raw call once."""
    from remixt_amd import queries
    R, MAX_CN = 4, 4
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=MAX_CN, num_chains=3, seed=4)
    ps = synthetic.make_init_params(e, R, MAX_CN)
    entry = queries.entry('path_entropy')
    rs = restarts.RestartSet(e, ps, MAX_CN, num_clones=3, quiet=True, seeds=list(range(R)), options={'fb_nv': 1})
    answers = {}
    try:
        rs.variational_update(2)
        b, models = rs.batch, rs.models
        m0 = models[0]
        maps = (m0.seg_fwd_remap, m0.seg_is_original, m0.is_telomere)
        for k, regions in enumerate((REGIONS, None, [])):
            want = posteriors.batch_path_entropy(b, 0, R, regions, *maps)
            got = rs.path_entropy(regions)
            _same(got, want, 'set %d' % k)
            answers[k] = got
            for r, m in enumerate(models):
                one = dict((key, v[0]) for key, v in posteriors.batch_path_entropy(b, r, 1, regions, *maps).items())
                _same(m.path_entropy(regions), one, 'model %d regions %d' % (r, k))
        # against the raw call and the sibling that walks the same adjacencies
        marg, step = b.path_entropy_raw(0, R)
        fwd = np.asarray(m0.seg_fwd_remap)
        assert np.array_equal(answers[0]['segment_entropy'], marg[:, fwd])
        assert np.array_equal(np.isnan(answers[0]['step_entropy']), np.isnan(rs.cn_change_prob()))
        assert answers[1]['path_entropy'].shape == (R, 1) and answers[2]['path_entropy'].shape == (R, 0)
        cs, ce = posteriors.chains_from_telomeres(m0.is_telomere)
        whole = sum(marg[:, z] + step[:, a:z].sum(axis=1) for a, z in zip(cs, ce))
        assert np.abs(answers[1]['path_entropy'][:, 0] - whole).max() <= len(fwd) * 1e-12
        assert (answers[0]['perplexity'] >= 1 - 1e-12).all() and (answers[0]['total_correlation'] >= -40e-12).all()
    finally:
        rs.close()
    g = restarts.RestartGroups(e, ps, MAX_CN, groups=2, num_clones=3, quiet=True, seeds=list(range(R)), options={'fb_nv': 1})
    try:
        g.variational_update(2)
        g.synchronize()
        parts = [part.path_entropy(REGIONS) for part in g.sets]
        got = g.path_entropy(REGIONS)
        _same(got, restarts._join(parts, shared=entry.shared), 'groups')
        for key in got:
            assert got[key].shape == answers[0][key].shape
    finally:
        g.close()
    dg = restarts.DatasetGroups([e, e], [ps[:2], ps[2:]], MAX_CN, seeds=[[0, 1], [2, 3]], num_clones=3, quiet=True, options={'fb_nv': 1})
    try:
        dg.variational_update(2)
        dg.synchronize()
        want = [part.path_entropy(REGIONS) for part in dg.parts]
        got = dg.path_entropy(REGIONS)
        assert len(got) == 2
        for d in range(2):
            _same(got[d], want[d], 'datasets %d' % d)
    finally:
        dg.close()
