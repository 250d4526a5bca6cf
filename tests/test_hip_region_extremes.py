"""Region extremes on the device (rmx_region_extremes / k_region_extremes): against the log-domain numpy twin on the
read-back framelogprob / log_transmat -- in probability and, because every column has its own scale, in the log domain --,
the identities that tie the columns to rmx_region_prob, the sampler, two state classes, the mixed transition model,
inserted segments, invariance to batching and grouping, two staging chunks, no side effects on the model, errors, the
public forms and the pipeline.

A crafted zero normaliser is left out: the siblings' tests show no way to make D(s') zero under positive mass that does not
go through set_array on the forward plane of a live batch, which none of them does."""
import numpy as np
import pytest

from remixt_amd import posteriors, synthetic
from tests import extremes_twin
from tests import helpers as H
from tests.test_hip_region_events import MASKS, Case
from tests.test_hip_sample_cn import GRIDS, _fitted, _model_state, _pipeline_case, _same_results

pytestmark = pytest.mark.gpu

U = 2. ** -53
COLS = (1, 5, 16)
# (mask, level table) of every constraint a query is run with: a clone's total, 'any', a reflected one; two with a mask
CONSTRAINTS = [(None, 'peak_total_1'), (None, 'peak_total_any'), (None, 'floor_total_1'), ('not_loh', 'peak_total_any'), ('not_subclonal', 'floor_total_1')]


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


class ExtCase(Case):
    def tables(self, ncol, first_level=0):
        levels, names = posteriors.level_tables(self.b.cn_classes, ncol, first_level)
        return levels, names, dict((k, levels[self.b.seg_class, i]) for i, k in enumerate(names))

    def ext(self, runs, ncol, constraints=CONSTRAINTS, r0=None, nr=1, first_level=0, constrain='own'):
        levels, names, _ = self.tables(ncol, first_level)
        q = np.array([[a, b, -1 if mk is None else MASKS.index(mk), names.index(lv)] for (a, b) in runs for (mk, lv) in constraints], dtype=np.int32)
        out = self.b.region_extremes_raw(self.r if r0 is None else r0, nr, q, self.masks, levels, self.constrain if constrain == 'own' else constrain, ncol)
        return out.reshape(nr, len(runs), len(constraints), ncol)

    def runs(self):
        """Case.queries() (one segment, two over a plain and over a breakend adjacency, the whole longest chain, a chain's start
        and a chain's end) and a 10-segment run of the longest chain (the chain itself where it is shorter)."""
        c = int(np.argmax(self.ce - self.cs))
        return self.queries() + [(int(self.cs[c]), int(min(self.cs[c] + 9, self.ce[c])))]

    def check(self, runs, cols=COLS, constraints=CONSTRAINTS, first_level=0, tag=''):
        """|e^F - e^twin| <= L 1e-9 in every column; |F - twin| <= L 1e-9 where the twin is >= -300; twin -inf -> -inf exactly;
        -inf -> the twin -inf or below -700.  Returns (worst error over bound, columns of whole-run queries in (-300, -20))."""
        worst, deep = 0., 0
        for K in cols:
            got = self.ext(runs, K, constraints, first_level=first_level)[0]
            _, _, lev_seg = self.tables(K, first_level)
            for i, (a, b) in enumerate(runs):
                L = b - a + 1
                for j, (mk, lv) in enumerate(constraints):
                    want = extremes_twin.logcolumns(self.twin, a, b, K, lev_seg[lv], None if mk is None else self.mask_seg[mk], self.constrain)
                    g = got[i, j]
                    assert not np.isnan(g).any(), (tag, K, a, b, mk, lv, g)
                    err = np.abs(np.exp(g) - np.exp(want))
                    loud = want >= -300
                    with np.errstate(invalid='ignore'):
                        lerr = np.where(loud, np.abs(g - want), 0.)
                    n_deep = int(((want > -300) & (want < -20)).sum())
                    deep += n_deep
                    worst = max(worst, err.max() / (L * 1e-9), lerr.max() / (L * 1e-9))
                    print('%s K %d run [%d, %d] mask %s level %s: max |P - twin| %.3e, max |F - twin| (twin >= -300) %.3e, %d columns in (-300, -20), F %s' % (
                        tag, K, a, b, mk, lv, err.max(), lerr.max(), n_deep, g))
                    assert (err <= L * 1e-9).all(), (tag, K, a, b, mk, lv, g, want)
                    assert (lerr <= L * 1e-9).all(), (tag, K, a, b, mk, lv, g, want)
                    assert (g[want == -np.inf] == -np.inf).all(), (tag, K, a, b, mk, lv, g, want)
                    assert (want[g == -np.inf] < -700).all(), (tag, K, a, b, mk, lv, g, want)
        print('%s worst error over bound: %.3e; columns in (-300, -20): %d' % (tag, worst, deep))
        return worst, deep


@pytest.fixture(scope='module')
def cases(hip):
    return dict(((N, M, c), ExtCase(_fitted(hip, N, M, c))) for N, M, c in GRIDS)


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_twin(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    assert case.S == {8: 165, 12: 355, 6: 457}[max_cn] and case.S % 64
    assert case.m.num_breakpoints > 0 and (case.bidx >= 0).any()
    b = case.b
    b.profile_reset(); b.profile_enable(1)
    case.ext(case.runs(), 16)
    prof = b.profile(); b.profile_enable(0)
    assert prof['k_region_extremes'][1] == 1 and prof['k_region_extremes'][0] > 0
    worst, _ = case.check(case.runs(), tag='S %d' % case.S)
    assert worst <= 1.
    # the whole longest chain alone: columns far below the top one keep their digits (a shared scale would lose them)
    c = int(np.argmax(case.ce - case.cs))
    _, deep = case.check([(int(case.cs[c]), int(case.ce[c]))], cols=(16,), tag='S %d whole chain' % case.S)
    assert deep >= 1
    # the model-level form
    levels, names, _ = case.tables(5)
    q = np.array([[a, b_, 1, 2] for a, b_ in case.queries()], dtype=np.int32)
    one = case.m.model.region_extremes(q, case.masks, levels, case.constrain, 5)
    assert one.shape == (len(q), 5) and np.array_equal(one, b.region_extremes_raw(case.r, 1, q, case.masks, levels, case.constrain, 5)[0])


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_identities(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    b, S, K = case.b, case.S, 16
    c = int(np.argmax(case.ce - case.cs))
    seg = np.arange(case.cs[c], case.ce[c] + 1)
    runs = [(int(a), int(e)) for a in seg for e in seg if a <= e]
    L = np.array([e - a + 1 for a, e in runs])
    zeros = np.zeros((b.cn_classes.shape[0], 1, S), dtype=np.int16)
    mks = [None, 'not_loh', 'not_subclonal', 'loh']
    q = np.array([[a, e, -1 if mk is None else MASKS.index(mk), 0] for a, e in runs for mk in mks], dtype=np.int32)
    # (i) a level table of zeros: every column is the mask-only event of rmx_region_prob; without a mask it is certain
    gz = b.region_extremes_raw(case.r, 1, q, case.masks, zeros, case.constrain, K)[0].reshape(len(runs), len(mks), K)
    gp = case.raw(runs, [(mk, None) for mk in mks])[0]
    err = np.abs(np.exp(gz) - np.exp(gp)[..., None])
    print('S %d: zero levels against the mask-only query: max |dP| %.3e' % (S, err.max()))
    assert (err <= L[:, None, None] * 1e-9).all()
    bound = L * (4 * S + 32) * U + 16 * U
    print('S %d: zero levels, no mask: max |F| %.3e over %d runs (bound of one segment %.3e)' % (S, np.abs(gz[:, 0]).max(), len(runs), bound.min()))
    assert (np.abs(gz[:, 0]) <= bound[:, None]).all()
    # (ii) a one-segment query is the sum of the marginals over the admitted states (4.10's bound for its one-segment identity)
    post = b.get_array(case.r, 'posterior_marginals')
    levels, names, lev_seg = case.tables(K)
    for mk, lv in CONSTRAINTS:
        one = case.ext([(n, n) for n in range(case.N)], K, [(mk, lv)])[0, :, 0]
        for j in range(K):
            adm = lev_seg[lv] <= j
            if mk is not None:
                adm = adm & case.mask_seg[mk]
            adm = np.where(case.constrain[:, None], adm, True)
            want = np.where(adm, post, 0.).sum(axis=1)
            with np.errstate(divide='ignore'):
                assert np.array_equal(one[:, j] == -np.inf, want == 0), (mk, lv, j)
                ok = want > 0
                tol = ((S + 4) + 3 * np.abs(np.log(want[ok]))) * U
            rel = np.abs(np.exp(one[ok, j]) / want[ok] - 1)
            assert (rel <= tol).all(), (mk, lv, j, rel.max())
    # (iii) column j is rmx_region_prob with the custom mask (mask and level <= j)
    sub = runs[::3]
    Ls = np.array([e - a + 1 for a, e in sub])
    for mk, lv in CONSTRAINTS:
        got = case.ext(sub, K, [(mk, lv)])[0, :, 0]
        custom = (levels[:, names.index(lv), None, :] <= np.arange(K)[None, :, None])
        if mk is not None:
            custom = custom & (case.masks[:, MASKS.index(mk), None, :] != 0)
        qq = np.array([[a, e, j, -1] for a, e in sub for j in range(K)], dtype=np.int32)
        ref = b.region_logprob_raw(case.r, 1, qq, custom.astype(np.uint8), None, case.constrain)[0].reshape(len(sub), K)
        err = np.abs(np.exp(got) - np.exp(ref))
        print('S %d: mask %s level %s against 16 custom-mask queries: max |dP| %.3e' % (S, mk, lv, err.max()))
        assert (err <= Ls[:, None] * 1e-9).all(), (mk, lv)
        # (iv) F does not decrease in j
        with np.errstate(invalid='ignore'):
            drop = np.where(np.isfinite(got[:, :-1]), got[:, :-1] - got[:, 1:], np.where(got[:, :-1] == -np.inf, -np.inf, np.nan))
        assert (drop <= (Ls * (4 * S + 32) * U)[:, None]).all(), (mk, lv, np.nanmax(drop))
    # (v) the columns are independent: 5 columns are the first 5 of 16, bit for bit, on a table that is not clipped
    raw_levels = levels.copy()      # (clipped at 15: above every total but the largest at 12 copies, and the same table in both calls)
    qq = np.array([[a, e, mi, names.index(lv)] for a, e in sub for mi, lv in ((-1, 'peak_total_1'), (-1, 'peak_total_any'), (1, 'peak_major_1'))], dtype=np.int32)
    g16 = b.region_extremes_raw(case.r, 1, qq, case.masks, raw_levels, case.constrain, 16)
    g5 = b.region_extremes_raw(case.r, 1, qq, case.masks, raw_levels, case.constrain, 5)
    assert np.array_equal(g5, g16[..., :5])
    assert (raw_levels[:, [names.index('peak_total_any')]] >= 5).any()


def test_against_the_sampler(hip):
    """peak_pmf and floor_pmf of the masked case of test_hip_region_events.test_against_the_sampler against 4 096 posterior
    samples (seed 99): every bin within 5 sqrt(p (1 - p) / 4096) + 1 / 4096."""
    from tests.test_hip_posterior_summary import _fitted as fitted_masked
    m = fitted_masked(hip, 30, 3, 8, sweeps=3, masked=True)
    NS, K = 4096, 16
    b, r = m.model._batch, m.model._r
    st = b.sample_states(r, 1, NS, [99]).astype(np.int64)[0]
    cn = np.asarray(b.cn_classes)[np.asarray(b.seg_class)[None, :], st]          # (NS, N1, M, 2)
    fwd = np.asarray(m.seg_fwd_remap)
    regions = [(0, 0), (3, 4), (2, 11), (0, m.N - 1), (12, 29)]
    informative = 0
    for quantity, clone in (('total', 'any'), ('total', 1), ('major', 2)):
        out = m.region_cn_extremes(regions, quantity=quantity, clone=clone, bins=K)
        v = posteriors._level_quantity(cn.reshape((1, -1) + cn.shape[2:]), quantity).reshape(NS, -1, cn.shape[2] - 1)
        for k, (i, j) in enumerate(regions):
            seg = fwd[i:j + 1]
            hi = (v[:, seg].max(axis=2) if clone == 'any' else v[:, seg, clone - 1]).max(axis=1)
            lo = (v[:, seg].min(axis=2) if clone == 'any' else v[:, seg, clone - 1]).min(axis=1)
            for name, smp in (('peak_pmf', hi), ('floor_pmf', lo)):
                freq = np.bincount(np.minimum(smp, K - 1), minlength=K) / NS
                P = out[name][k]
                tol = 5 * np.sqrt(P * (1 - P) / NS) + 1. / NS
                informative += int(((P > 0.01) & (P < 0.99)).sum())
                assert (np.abs(freq - P) <= tol).all(), (quantity, clone, i, j, name, freq, P)
    print('informative (region, bin) pairs: %d' % informative)
    assert informative >= 3


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
        case = ExtCase(m, batch=b, r=0)
        levels, names, _ = case.tables(5)
        i = names.index('peak_total_1')
        assert np.array_equal(levels[1, i], np.minimum(levels[0, i].astype(int) + 2, 4))      # the level differs per class
        worst, _ = case.check(case.runs(), cols=(5,), tag='two classes')
        assert worst <= 1.
        # (a kernel that took class 0's levels everywhere would admit total 0 at the odd segments)
        odd = case.ext([(n, n) for n in range(1, N, 2)], 5, [(None, 'peak_total_1')])[0, :, 0]
        assert (odd[case.constrain[1::2], :2] == -np.inf).all() and np.isfinite(odd[:, 4]).all()
    finally:
        b.close()


def test_mixed_transition_model(hip):
    """Restarts 0 and 3 keep their model-0 snapshot, restarts 1 and 2 take theirs under model 1: a call over 0 .. 3 has three
    launches and equals the single-restart calls bit for bit; restarts 0 and 1 agree with the twin on their own snapshot."""
    from tests.test_hip_query_driver import _restart_set
    rs = _restart_set(4)
    try:
        b = rs.batch
        b.transition_model = 1
        b.update_p_cn(1, 3)
        cs_ = [ExtCase(rs.models[r]) for r in (0, 1)]
        case = cs_[0]
        runs = case.runs()
        call = lambda r0, nr: case.ext(runs, 16, r0=r0, nr=nr)
        b.profile_reset(); b.profile_enable(1)
        full = call(0, 4)
        launches = b.profile()['k_region_extremes'][1]; b.profile_enable(0)
        assert launches == 3
        assert len(np.unique(full.reshape(4, -1), axis=0)) > 1
        for r in range(4):
            assert np.array_equal(call(r, 1)[0], full[r]), r
        assert np.array_equal(call(1, 3), full[1:])
        for c in cs_:
            worst, _ = c.check(runs, cols=(16,), tag='mixed model, restart %d' % c.r)
            assert worst <= 1.
    finally:
        rs.close()


def test_inserted_segments(hip):
    """Two breakends on one boundary: the model inserts a zero-length segment there.  Neither mask nor level binds it: a
    query of it alone is certain in every column, and a run through it changes when constrain is dropped."""
    e = synthetic.make_experiment(60, num_clones=3, max_copy_number=4, num_chains=3, seed=7)
    e.breakpoints = H.add_shared_boundary_breakpoints(e)
    m, h, _ = H.make_model(hip, M=3, max_cn=4, experiment=e)
    H.attach(m, h)
    m.model.allele_likelihood_mask = np.zeros(m.model.num_segments, dtype=int)      # (events of intermediate probability)
    m.variational_update(); m.variational_update()
    case = ExtCase(m)
    assert m.N1 > m.N and not case.constrain.all()
    dummy = int(np.flatnonzero(~case.constrain & (np.arange(m.N1) > 0) & (case.tel == 0))[0])
    assert case.constrain[dummy - 1] and case.constrain[dummy + 1]
    runs = [(dummy - 1, dummy + 1), (dummy, dummy), (dummy, dummy + 1), (dummy - 3, dummy + 2)]
    worst, _ = case.check(runs, cols=(1, 6), tag='inserted segment')
    assert worst <= 1.
    K = 6
    alone = case.ext([(dummy, dummy)], K)[0, 0]
    assert (np.abs(alone) <= (4 * case.S + 32) * U).all()                   # nothing binds: certain in every column
    bound = case.ext([(dummy, dummy)], K, constrain=None)[0, 0]
    assert (bound[0, :2] < -1e-6).all()                                     # with every segment bound the low columns are not
    through, through_all = case.ext(runs[:1], K)[0, 0], case.ext(runs[:1], K, constrain=None)[0, 0]
    assert (through_all <= through + 3 * (4 * case.S + 32) * U).all() and (through_all[0, :2] < through[0, :2] - 1e-9).any()
    # the experiment pair around it, through region_cn_extremes: the inserted segment does not count towards the peak
    i = int(m.seg_rev_remap[dummy - 1])
    assert m.seg_fwd_remap[i] == dummy - 1 and m.seg_fwd_remap[i + 1] == dummy + 1
    out = m.region_cn_extremes([(i, i + 1)], quantity='total', clone=1, bins=K)
    _, _, lev_seg = case.tables(K)
    want = extremes_twin.logcolumns(case.twin, dummy - 1, dummy + 1, K, lev_seg['peak_total_1'], None, case.constrain)
    assert np.abs(out['peak_cdf'][0] - np.exp(want)).max() <= 3e-9


def test_invariance(hip):
    from remixt_amd.restarts import RestartGroups, RestartSet
    e = synthetic.make_experiment(80, num_clones=3, max_copy_number=4, num_chains=3, seed=4)
    ps = synthetic.make_init_params(e, 4, 4)
    rs = RestartSet(e, ps, 4, num_clones=3, quiet=True, seeds=list(range(4)))
    rs.variational_update(2)
    b, m = rs.batch, rs.models[0]
    masks, _ = posteriors.event_tables(b.cn_classes)
    K = 6
    levels, names = posteriors.level_tables(b.cn_classes, K)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    regions = [(i, j) for i in range(0, 70, 7) for j in (i, i + 1, i + 9)]
    runs, _, constrain = posteriors.region_queries(regions, m.seg_fwd_remap, m.seg_is_original, cs, ce)
    q = np.array([[a, e_, mi, li] for a, e_ in runs for mi, li in ((-1, 0), (1, 2), (5, names.index('floor_minor_any')))], dtype=np.int32)
    call = lambda r0, nr, qq: b.region_extremes_raw(r0, nr, qq, masks, levels, constrain, K)
    full = call(0, 4, q)
    assert full.shape == (4, len(q), K) and not np.array_equal(full[0], full[1]) and not np.isnan(full).any()
    for r in range(4):
        assert np.array_equal(call(r, 1, q)[0], full[r])
    assert np.array_equal(call(1, 2, q), full[1:3])
    for i in range(0, len(q), 5):
        assert np.array_equal(call(0, 4, q[i:i + 1])[:, 0], full[:, i])
    assert np.array_equal(call(0, 4, q[::-1].copy()), full[:, ::-1])
    per_set = rs.region_cn_extremes(regions, bins=K)
    one = rs.models[2].region_cn_extremes(regions, bins=K)
    per_clone, one_clone = rs.region_clone_extremes(regions, bins=K), rs.models[2].region_clone_extremes(regions, bins=K)
    for k in ('peak_cdf', 'peak_pmf', 'floor_cdf', 'floor_pmf', 'peak_q50', 'floor_q95'):
        assert per_set[k].shape[:2] == (4, len(regions)) and np.array_equal(per_set[k][2], one[k]), k
    for k in posteriors.EXTREME_ARRAYS:
        assert per_clone[k].shape == (4, len(regions), 2, K) and np.array_equal(per_clone[k][2], one_clone[k]), k
        assert np.abs(per_clone[k].sum(axis=-1) - 1).max() <= 1e-9, k
    rs.close()
    groups = RestartGroups(e, ps, 4, groups=2, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    single = RestartGroups(e, ps, 4, groups=1, num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    for g in (groups, single):
        g.variational_update(2)
    a, c = groups.region_cn_extremes(regions, bins=K), single.region_cn_extremes(regions, bins=K)
    for k in ('peak_cdf', 'floor_pmf', 'peak_q95'):
        assert a[k].shape[:2] == (4, len(regions)) and np.array_equal(a[k], c[k]), k
    groups.close(); single.close()


def test_two_staging_chunks(hip):
    """One restart, 16 columns, about 470 000 one-segment queries: more than one chunk of the 64 MiB staging buffer holds."""
    m = _fitted(hip, 60, 3, 8)
    b, r = m.model._batch, m.model._r
    levels, names = posteriors.level_tables(b.cn_classes, 16)
    N = b.num_segments
    nq = (64 << 20) // (16 * 8 + 16) + 4000
    assert 465000 < nq < 475000
    q = np.zeros((nq, 4), dtype=np.int32)
    q[:, 0] = q[:, 1] = np.arange(nq) % N
    q[:, 2], q[:, 3] = -1, names.index('peak_total_any')
    b.profile_reset(); b.profile_enable(1)
    big = b.region_extremes_raw(r, 1, q, None, levels, None, 16)[0]
    launches = b.profile()['k_region_extremes'][1]; b.profile_enable(0)
    assert launches == 2
    first = b.region_extremes_raw(r, 1, q[:N], None, levels, None, 16)[0]
    assert np.array_equal(big[:nq // N * N].reshape(-1, N, 16), np.broadcast_to(first, (nq // N, N, 16)))
    assert np.array_equal(big[nq // N * N:], first[:nq % N])


def test_no_side_effects(hip):
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    before = _model_state(m1)
    out = m1.region_cn_extremes([(0, 10), (5, 5), (20, 49)], bins=16)
    assert out['peak_pmf'].shape == (3, 16) and out['bins'] == 16
    after = _model_state(m1)
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    for m in (m1, m2):
        m.variational_update()
    s1, s2 = _model_state(m1), _model_state(m2)
    for k in s1:
        assert np.array_equal(s1[k], s2[k], equal_nan=True), k
    assert m1.model.calculate_elbo() == m2.model.calculate_elbo()


def test_errors(hip):
    from remixt_amd import bpmodel
    m, h, e = H.make_model(hip, N=30, M=3, max_cn=3)
    H.attach(m, h)
    b, r = m.model._batch, m.model._r
    masks, _ = posteriors.event_tables(b.cn_classes)
    levels, names = posteriors.level_tables(b.cn_classes, 4)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    ok = [[int(cs[0]), int(cs[0]) + 1, 0, 0]]
    with pytest.raises(ValueError, match='update_p_cn'):
        b.region_extremes_raw(r, 1, ok, masks, levels, None, 4)
    assert bpmodel.last_error_restarts() == [r]
    with pytest.raises(ValueError, match='update_p_cn'):
        m.region_cn_extremes([(0, 3)])
    m.variational_update()
    N, T = b.num_segments, len(names)
    lib, handle = b._lib, b._handle
    b.profile_reset(); b.profile_enable(1)
    assert b.region_extremes_raw(r, 1, ok, masks, levels, None, 4).shape == (1, 1, 4)
    launches = b.profile()['k_region_extremes'][1]
    assert launches == 1
    negative = levels.copy(); negative[-1, -1, -1] = -1
    bad = [(ok, 0, levels, 'columns'), (ok, 17, levels, 'columns'), (ok, -1, levels, 'columns'), (ok + [[0, 1, -1, -1]], 4, levels, 'level index'),
           (ok + [[0, 1, -1, T]], 4, levels, 'level index'), (ok, 4, negative, 'level entry is negative'), (ok + [[3, 2, -1, 0]], 4, levels, 'first <= last'),
           (ok + [[int(ce[0]), int(ce[0]) + 1, -1, 0]], 4, levels, 'chain end'), (ok + [[int(cs[0]), int(ce[1]), -1, 0]], 4, levels, 'chain end'),
           (ok + [[0, N, -1, 0]], 4, levels, 'first <= last'), (ok + [[-1, 0, -1, 0]], 4, levels, 'first <= last'), (ok + [[0, 1, len(MASKS), 0]], 4, levels, 'mask index'),
           (ok + [[0, 1, -2, 0]], 4, levels, 'mask index')]
    import ctypes as C
    for q, K, lv, text in bad:
        # through the C entry point with an output buffer of its own: refused, and the buffer is untouched
        qa, args, _keep = b._region_args(q, masks, lv, None)
        obuf = np.full((1, len(q), 16), 7.25)
        rc = lib.rmx_region_extremes(handle, r, 1, *args, K, obuf.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == 5 and (obuf == 7.25).all(), (q, K, text, rc)
        with pytest.raises(ValueError, match='^bad argument: .*' + text):
            b.region_extremes_raw(r, 1, q, masks, lv, None, K)
        assert bpmodel.last_error_restarts() == []
        assert b.profile()['k_region_extremes'][1] == launches, (q, K)      # nothing was launched
    for r0, nr in ((-1, 1), (0, 0), (0, 2)):
        qa, args, _keep = b._region_args(ok, masks, levels, None)
        obuf = np.full((2, 1, 4), 7.25)
        assert lib.rmx_region_extremes(handle, r0, nr, *args, 4, obuf.ctypes.data_as(C.POINTER(C.c_double))) == 5 and (obuf == 7.25).all()
    assert b.profile()['k_region_extremes'][1] == launches
    b.profile_enable(0)
    with pytest.raises(ValueError, match='bins'):
        m.region_cn_extremes([(0, 3)], bins=17)
    with pytest.raises(ValueError, match='clone'):
        m.region_cn_extremes([(0, 3)], clone=3)
    with pytest.raises(ValueError, match='quantity'):
        m.region_cn_extremes([(0, 3)], quantity='depth')
    from oracle import oracle
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError):
        mo.region_cn_extremes([(0, 3)])


def test_public_forms(hip, cases):
    """BreakpointModel.region_cn_extremes against the twin: regions across chain ends (the pieces' columns multiply), the
    reflected table behind floor_cdf, a slid window, and amplification_prob."""
    case = cases[GRIDS[0]]
    m = case.m
    regions = [(0, 0), (2, 7), (0, m.N - 1), (m.N - 3, m.N - 1), (5, 40)]
    runs, piece_region, _ = posteriors.region_queries(regions, m.seg_fwd_remap, m.seg_is_original, case.cs, case.ce)
    assert len(runs) > len(regions)
    for quantity, clone, K, first in (('total', 'any', 16, 0), ('total', 1, 6, 2), ('minor', 2, 4, 0)):
        out = m.region_cn_extremes(regions, quantity=quantity, clone=clone, bins=K, first_level=first)
        _, _, lev_seg = case.tables(K, first)
        F = np.zeros((2, len(regions), K))
        for (a, z), k in zip(runs, piece_region):
            for o, orient in enumerate(('peak', 'floor')):
                F[o, k] += extremes_twin.logcolumns(case.twin, int(a), int(z), K, lev_seg[posteriors.level_name(orient, quantity, clone)], None, case.constrain)
        want = posteriors.extremes_summary(F[0], F[1][:, ::-1], first)
        Lr = np.array([sum(z - a + 1 for (a, z), k in zip(runs, piece_region) if k == i) for i in range(len(regions))])
        for key in ('peak_cdf', 'floor_cdf'):
            assert (np.abs(out[key] - want[key]) <= Lr[:, None] * 1e-9).all(), (quantity, clone, key)
        for key in ('peak_pmf', 'floor_pmf'):
            assert (np.abs(out[key] - want[key]) <= 2 * Lr[:, None] * 1e-9).all(), (quantity, clone, key)
            assert ((out[key] >= 0) & (out[key] <= 1)).all() and np.abs(out[key].sum(axis=1) - 1).max() <= 1e-9
        assert out['peak_cdf'][:, -1].min() >= 1 - 1e-9 and out['floor_cdf'][:, 0].min() >= 1 - 1e-9
        assert (out['peak_q05'] <= out['peak_q50']).all() and (out['peak_q50'] <= out['peak_q95']).all() and (out['floor_q50'] <= out['peak_q50']).all()
        assert out['peak_q05'].min() >= first and out['peak_q95'].max() <= first + K - 1
        amp = posteriors.amplification_prob(out, first + 2)
        assert np.abs(amp - (1 - out['peak_cdf'][:, 1])).max() <= 1e-15
    # (RestartSet / RestartGroups: test_invariance ties them to this form bit for bit)


def test_pipeline_cn_region_extremes(hip, tmp_path):
    from remixt_amd import restarts, workflow
    from remixt_amd.analysis import pipeline
    import pickle
    e, config, init_params = _pipeline_case()
    ids = sorted(init_params)
    seeds = [100 + i for i in ids]
    cn_regions = [('geneA', 10, 14), ('arm', 0, 250), ('seg', 77, 77), ('pair', 300, 301)]
    K = posteriors.EXTREME_BINS
    with pytest.raises(ValueError, match='cn_regions'):
        pipeline.fit_restarts(e, init_params, dict(config, cn_region_extremes=True), seeds=seeds, groups=2)
    base = pipeline.fit_restarts(e, init_params, dict(config, cn_regions=cn_regions), seeds=seeds, groups=2)
    on = pipeline.fit_restarts(e, init_params, dict(config, cn_regions=cn_regions, cn_region_extremes=True), seeds=seeds, groups=2)
    assert not any('region_cn_extremes' in res for res in base.values())
    strip = lambda results: dict((i, dict((k, v) for k, v in res.items() if k not in ('region_events', 'region_cn_extremes'))) for i, res in results.items())
    _same_results(strip(base), strip(on))
    for i in ids:
        ex = on[i]['region_cn_extremes']
        assert ex['names'] == ['geneA', 'arm', 'seg', 'pair'] and ex['bins'] == K and sorted(ex) == ['bins', 'floor_total_pmf', 'names', 'peak_total_pmf']
        for k in posteriors.EXTREME_ARRAYS:
            assert ex[k].shape == (4, 2, K) and ((ex[k] >= 0) & (ex[k] <= 1)).all(), (i, k)
            assert np.abs(ex[k].sum(axis=-1) - 1).max() <= 1e-9, (i, k)
        assert np.abs(ex['peak_total_pmf'][2] - ex['floor_total_pmf'][2]).max() <= 3e-9      # one segment: its peak is its lowest value
    one = pipeline.fit(e, init_params[ids[1]], dict(config, cn_regions=cn_regions, cn_region_extremes=True), quiet=True, init_id=ids[1])
    assert one['region_cn_extremes']['peak_total_pmf'].shape == (4, 2, K) and one['region_cn_extremes']['names'] == ex['names']
    dist = restarts.fit_restarts_distributed(e, [init_params[i] for i in ids], 4, num_clones=3, num_em_iter=config['num_em_iter'],
                                             num_update_iter=config['num_update_iter'], seeds=seeds, quiet=True, cn_regions=cn_regions,
                                             cn_region_extremes=True, **pipeline._model_kwargs(e, config))
    for j, i in enumerate(ids):
        assert dist[j]['region_cn_extremes']['names'] == ex['names'] and dist[j]['region_cn_extremes']['bins'] == K
        for k in posteriors.EXTREME_ARRAYS:
            assert np.array_equal(dist[j]['region_cn_extremes'][k], on[i]['region_cn_extremes'][k]), (i, k)
    exp_file = str(tmp_path / 'experiment.pickle')
    with open(exp_file, 'wb') as f:
        pickle.dump(e, f)
    workflow.fit_model(exp_file, str(tmp_path / 'r.store'), dict(config, cn_regions=cn_regions, cn_region_extremes=True), None, seeds=seeds)
    with pipeline._Store(str(tmp_path / 'r.store'), 'r') as st:
        for i in sorted(st['stats']['init_id']):
            for k in posteriors.EXTREME_ARRAYS:
                v = np.asarray(st['solutions/solution_%d/region_%s' % (i, k)])
                assert v.shape == (4, 2 * K) and np.array_equal(v.reshape(4, 2, K), on[i]['region_cn_extremes'][k]), (i, k)
    workflow.fit_model(exp_file, str(tmp_path / 'r0.store'), dict(config, cn_regions=cn_regions), None, seeds=seeds)
    with pipeline._Store(str(tmp_path / 'r0.store'), 'r') as st:
        assert not any('total_pmf' in k for k in st.keys())
