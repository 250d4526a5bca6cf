"""Restart overlap on the device (rmx_restart_overlap / k_restart_overlap): against the log-domain numpy twin on the
read-back framelogprob / log_transmat of both restarts, the exact identities of the recursion, invariance to the pair list,
the query batch, the grouping of the restarts (a pair that straddles two batches) and the chunking, the non-current
transition model, errors, no side effects on the models, and the point of it: two fits that differ by the order of their
tumour clones are recognised as one solution."""
import numpy as np
import pytest

from remixt_amd import posteriors, synthetic
from tests import overlap_twin
from tests.test_hip_region_events import Case
from tests.test_hip_sample_cn import GRIDS, _model_state

pytestmark = pytest.mark.gpu

U = 2. ** -53
PAIRS = [(0, 1), (0, 2), (1, 2)]
# the tumour depth split over the tumour clones, one row per restart: three restarts with different h
SPLITS = {3: [(0.45, 0.55), (0.3, 0.7), (0.6, 0.4)], 4: [(0.5, 0.3, 0.2), (0.2, 0.3, 0.5), (0.4, 0.35, 0.25)]}


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


def _restart_set(N, M, max_cn, seed=0):
    """Three restarts with different h over a synthetic experiment with three chains and breakpoints: two variational sweeps,
    no M-step."""
    from remixt_amd.restarts import RestartSet
    e = synthetic.make_experiment(N, num_clones=M, max_copy_number=max_cn, num_chains=3, seed=seed)
    ps = synthetic.make_init_params(e, 3, max_cn, num_clones=M)
    h = np.array([[p['h_normal']] + [p['h_tumour'] * f for f in fr] for p, fr in zip(ps, SPLITS[M])])
    rs = RestartSet(e, ps, max_cn, num_clones=M, quiet=True, seeds=[0, 1, 2], h_init=h)
    rs.variational_update(2)
    return rs


class OvCase(object):
    """A set of three restarts with everything the comparisons share: the runs, the clone maps and their state tables, the
    read-back arrays of every restart and the twin's values (computed once)."""

    def __init__(self, rs):
        self.rs, self.b = rs, rs.batch
        b = self.b
        self.ev = Case(rs.models[0])
        self.N, self.S = b.num_segments, b.num_cn_states
        self.cs, self.ce = self.ev.cs, self.ev.ce
        self.runs = self.ev.queries()
        self.maps = posteriors.clone_permutations(b.num_clones)
        self.tables = posteriors.state_permutation_tables(b.cn_classes, self.maps)
        self.inv = [self.maps.index(tuple(int(v) for v in np.argsort(p))) for p in self.maps]
        self.perm_seg = self.tables[:, np.asarray(b.seg_class)].astype(np.int64)      # (maps, N, S)
        R = len(rs.models)
        self.post = [b.get_array(r, 'posterior_marginals') for r in range(R)]
        self._sides, self._want = {}, {}

    def side(self, r):
        if r not in self._sides:
            self._sides[r] = overlap_twin.Side(self.b.get_array(r, 'framelogprob'), self.b.get_array(r, 'log_transmat'), self.cs, self.ce)
        return self._sides[r]

    def want(self, i, j, a, e, mp):
        """(mode 0, mode 1) of the twin"""
        key = (i, j, a, e, mp)
        if key not in self._want:
            self._want[key] = overlap_twin.OverlapTwin(self.side(i), self.side(j)).logz_modes(a, e, self.perm_seg[mp])
        return self._want[key]

    def raw(self, pairs, runs, mode, maps=None):
        """(pairs, runs, maps)"""
        maps = list(range(len(self.maps))) if maps is None else maps
        q = np.array([[a, e, mp, 0] for (a, e) in runs for mp in maps], dtype=np.int32)
        out = self.b.restart_overlap_raw(None, pairs, q, self.tables, mode)
        return out.reshape(len(pairs), len(runs), len(maps))

    def check_against_twin(self, tag):
        worst = 0.
        for mode in (0, 1):
            got = self.raw(PAIRS, self.runs, mode)
            for k, (i, j) in enumerate(PAIRS):
                for x, (a, e) in enumerate(self.runs):
                    L = e - a + 1
                    for mp in range(len(self.maps)):
                        want = self.want(i, j, a, e, mp)[mode]
                        err = abs(np.exp(got[k, x, mp]) - np.exp(want))
                        worst = max(worst, err / (2 * L))
                        print('%s pair %s run [%d, %d] map %s mode %d: log Z %.17g (twin %.17g), |Z - twin| %.3e' % (
                            tag, (i, j), a, e, self.maps[mp], mode, got[k, x, mp], want, err))
                        assert err <= 2 * L * 1e-9, (tag, i, j, a, e, mp, mode, got[k, x, mp], want)
        print('%s worst |Z - twin| / 2 L: %.3e' % (tag, worst))


@pytest.fixture(scope='module')
def cases(hip):
    made = {}

    def get(grid):
        if grid not in made:
            made[grid] = OvCase(_restart_set(*grid))
        return made[grid]
    yield get
    for c in made.values():
        c.rs.close()


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_twin(hip, cases, N, M, max_cn):
    case = cases((N, M, max_cn))
    assert case.S == {8: 165, 12: 355, 6: 457}[max_cn] and case.S % 64
    assert (case.ev.bidx >= 0).any() and len(case.cs) == 3
    h = np.array([m.model.h for m in case.rs.models])
    assert len(np.unique(h.round(12), axis=0)) == 3
    b = case.b
    b.profile_reset(); b.profile_enable(1)
    case.check_against_twin('S %d' % case.S)
    prof = b.profile(); b.profile_enable(0)
    # one launch per mode (every snapshot is under the current model); one chain's kernel is not what ran
    assert prof['k_restart_overlap'][1] == 2 and prof['k_restart_overlap'][0] > 0 and 'k_region_prob' not in prof


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_identities(hip, cases, N, M, max_cn):
    case = cases((N, M, max_cn))
    S, nm = case.S, len(case.maps)
    # A = B under the identity: BC = 1 on every run -- the case's runs and every pair of segments of the longest chain
    c = int(np.argmax(case.ce - case.cs))
    seg = np.arange(case.cs[c], case.ce[c] + 1)
    runs = case.runs + [(int(a), int(e)) for a in seg for e in seg if a <= e]
    own = [(r, r) for r in range(3)]
    lz = case.raw(own, runs, 0, maps=[0])[:, :, 0]
    L = np.array([e - a + 1 for a, e in runs])
    print('S %d: A = B, identity, mode 1/2: max |log Z| / (L (4 S + 40) u) = %.3f' % (S, (np.abs(lz) / (L * (4 * S + 40) * U)).max()))
    assert (np.abs(lz) <= L * (4 * S + 40) * U).all(), np.abs(lz).max()
    # a one-segment query is the sum over the states of the two marginals' product
    allp = own + PAIRS
    one = [(n, n) for n in range(case.N)]
    for mode in (0, 1):
        got = case.raw(allp, one, mode)
        worst = 0.
        for k, (i, j) in enumerate(allp):
            for mp in range(nm):
                pa = case.post[i]
                pb = np.take_along_axis(case.post[j], case.perm_seg[mp], axis=1)
                want = (np.sqrt(pa) * np.sqrt(pb)).sum(axis=1) if mode == 0 else (pa * pb).sum(axis=1)
                with np.errstate(divide='ignore'):
                    assert np.array_equal(got[k, :, mp] == -np.inf, want == 0), (i, j, mp, mode)
                ok = want > 0
                rel = np.abs(np.exp(got[k, ok, mp].astype(np.longdouble)) / want[ok].astype(np.longdouble) - 1)
                worst = max(worst, float(rel.max()))
                assert (rel <= (S + 8) * U).all(), (i, j, mp, mode, float(rel.max()) / U, got[k, ok, mp][np.argmax(rel)])
        print('S %d: one segment, mode %d: worst relative error %.1f u (bound %d u)' % (S, mode, worst / U, S + 8))
    # (A, B, pi) against (B, A, the inverse of pi), and Cauchy-Schwarz
    swapped = [(j, i) for i, j in PAIRS]
    for mode in (0, 1):
        ab, ba = case.raw(PAIRS, case.runs, mode), case.raw(swapped, case.runs, mode)
        Lr = np.array([e - a + 1 for a, e in case.runs])[None, :, None]
        d = np.abs(ab - ba[:, :, case.inv])
        both = np.isfinite(ab)
        assert np.array_equal(both, np.isfinite(ba[:, :, case.inv]))
        print('S %d: (A, B, pi) against (B, A, inverse), mode %d: max |d log Z| / (L (4 S + 40) u) = %.3f' % (
            S, mode, (np.where(both, d, 0.) / (Lr * (4 * S + 40) * U)).max()))
        assert (np.where(both, d, 0.) <= Lr * (4 * S + 40) * U).all()
    slack = np.array([e - a + 1 for a, e in case.runs]) * (4 * S + 40) * U
    bc = case.raw(PAIRS, case.runs, 0)
    assert (bc <= slack[None, :, None]).all(), bc.max()
    co = case.raw(PAIRS, case.runs, 1)
    self_co = case.raw(own, case.runs, 1, maps=[0])[:, :, 0]
    for k, (i, j) in enumerate(PAIRS):
        # (the collision probability of q_B does not change under a relabelling of its states)
        assert (co[k] <= 0.5 * (self_co[i] + self_co[j])[:, None] + slack[:, None]).all(), (i, j)
    assert (self_co <= slack[None]).all()


def test_shape_of_the_call(hip, cases):
    """A (pair, query) result is the same bits alone, in a batch of all pairs and all queries, in any order, across two restart
    groups -- a pair that straddles them reads two batches -- and in a call that runs in several chunks."""
    from remixt_amd.restarts import RestartGroups, RestartSet
    case = cases(GRIDS[0])
    nm = len(case.maps)
    for mode in (0, 1):
        full = case.raw(PAIRS, case.runs, mode)
        assert len(np.unique(full.reshape(len(PAIRS), -1), axis=0)) == len(PAIRS)
        for k, pair in enumerate(PAIRS):
            assert np.array_equal(case.raw([pair], case.runs, mode), full[k:k + 1])
            for x, run in enumerate(case.runs):
                for mp in range(nm):
                    assert np.array_equal(case.raw([pair], [run], mode, maps=[mp])[0, 0, 0], full[k, x, mp]), (pair, run, mp)
        assert np.array_equal(case.raw(PAIRS[::-1] + PAIRS, case.runs[::-1], mode), np.concatenate([full[::-1], full])[:, ::-1])
    # restart groups: the same fits in one batch, and in two batches of 2 + 2 restarts
    e = synthetic.make_experiment(80, num_clones=3, max_copy_number=4, num_chains=3, seed=4)
    ps = [synthetic.make_init_params(e, 12, 4)[i] for i in (0, 3, 6, 9)]      # (four tumour mixes: different h)
    regions = [(i, j) for i in range(0, 70, 14) for j in (i, i + 9)]
    kw = dict(num_clones=3, quiet=True, seeds=list(range(4)), options={'fb_nv': 1})
    rs = RestartSet(e, ps, 4, **kw)
    groups = RestartGroups(e, ps, 4, groups=2, **kw)
    try:
        rs.variational_update(2); groups.variational_update(2)
        assert len(groups.sets) == 2 and [len(s.models) for s in groups.sets] == [2, 2]
        one, two = rs.restart_overlap(regions), groups.restart_overlap(regions)
        assert [tuple(p) for p in one['pairs']] == [(i, j) for i in range(4) for j in range(i + 1, 4)]      # (0, 2) .. (1, 3) straddle
        assert one['log_overlap'].shape == (6, len(regions) + 1, 2) and one['self_log_coincidence'].shape == (4, len(regions) + 1)
        assert np.isfinite(one['log_overlap']).all() and len(np.unique(one['log_overlap'][:, -1, 0])) == 6
        for k in ('pairs', 'log_overlap', 'log_coincidence', 'clone_map', 'hellinger', 'distance_rate', 'self_log_coincidence'):
            assert np.array_equal(one[k], two[k]), k
        assert one['clone_maps'] == two['clone_maps'] == [(0, 1, 2), (0, 2, 1)]
        # the straddling pair the other way round: A in the second batch, B in the first
        back = groups.restart_overlap(regions, pairs=[(3, 0), (2, 2)], clone_maps=[(0, 2, 1)])
        fwd = rs.restart_overlap(regions, pairs=[(3, 0), (2, 2)], clone_maps=[(0, 2, 1)])
        assert np.array_equal(back['log_overlap'], fwd['log_overlap']) and np.array_equal(back['log_coincidence'], fwd['log_coincidence'])
        assert ((one['hellinger'] >= 0) & (one['hellinger'] <= 1)).all() and (one['distance_rate'] >= -1e-12).all()
        # several chunks: 64 pair rows and more one-segment queries than (64 MiB) // (64 * 8 + 16) of them
        b = rs.batch
        tables = posteriors.state_permutation_tables(b.cn_classes, one['clone_maps'])
        pairs = [(i, j) for i in range(4) for j in range(4)] * 4
        chunk = (64 << 20) // (len(pairs) * 8 + 16)
        N1 = b.num_segments
        short = np.array([[n, n, mp, 0] for n in range(N1) for mp in (0, 1)], dtype=np.int32)
        many = np.tile(short, (chunk // len(short) + 2, 1))
        assert chunk < len(many) < 2 * chunk
        b.profile_reset(); b.profile_enable(1)
        big = b.restart_overlap_raw(None, pairs, many, tables, 0)
        launches = b.profile()['k_restart_overlap'][1]; b.profile_enable(0)
        assert launches == 2
        ref = b.restart_overlap_raw(None, pairs[:16], short, tables, 0)
        assert np.array_equal(big.reshape(4, 16, -1, len(short)), np.broadcast_to(ref[None, :, None, :], (4, 16, len(many) // len(short), len(short))))
    finally:
        rs.close(); groups.close()


def test_other_transition_model(hip):
    """Every snapshot under the non-current transition model: the plain weights come from that model's log table
    (exp(trans_value), no Wb rows).  A pair whose snapshots are of different models is refused with nothing queued."""
    from remixt_amd import bpmodel
    rs = _restart_set(40, 3, 4, seed=3)
    try:
        b = rs.batch
        T0 = b.get_array(0, 'log_transmat')
        b.transition_model = 1
        assert np.array_equal(b.get_array(0, 'log_transmat'), T0)         # the snapshots stay the model-0 ones
        case = OvCase(rs)
        b.profile_reset(); b.profile_enable(1)
        case.check_against_twin('other model')
        assert b.profile()['k_restart_overlap'][1] == 2
        own = case.raw([(1, 1)], case.runs, 0, maps=[0])[0, :, 0]
        L = np.array([e - a + 1 for a, e in case.runs])
        assert (np.abs(own) <= L * (4 * case.S + 40) * U).all()
        # restart 1 takes a snapshot under model 1: pairs with it are of two models
        b.update_p_cn(1, 2)
        before = b.profile()['k_restart_overlap'][1]
        for pairs, named in (([(0, 2), (0, 1)], 'pair 1 \\(restarts 0, 1\\)'), ([(1, 2)], 'pair 0 \\(restarts 1, 2\\)')):
            with pytest.raises(ValueError, match='^restart_overlap: the snapshots of ' + named + ' were taken under different transition models$'):
                case.raw(pairs, case.runs, 0)
            assert bpmodel.last_error_restarts() == []
        assert b.profile()['k_restart_overlap'][1] == before              # nothing was queued
        # pairs of one model each still run in one call: (0, 2) under model 0 on the log table, (1, 1) under model 1 on Wb rows
        mixed = case.raw([(1, 1), (0, 2), (1, 1)], case.runs, 0, maps=[0])[:, :, 0]
        assert b.profile()['k_restart_overlap'][1] == before + 2; b.profile_enable(0)
        assert (np.abs(mixed[[0, 2]]) <= L * (4 * case.S + 40) * U).all() and np.array_equal(mixed[0], mixed[2])
        for x, (a, e) in enumerate(case.runs):
            assert abs(np.exp(mixed[1, x]) - np.exp(case.want(0, 2, a, e, 0)[0])) <= 2 * (e - a + 1) * 1e-9
    finally:
        rs.close()


def test_errors(hip, cases):
    from remixt_amd import bpmodel
    from remixt_amd.restarts import RestartSet
    case = cases(GRIDS[0])
    b, tables = case.b, case.tables
    N, S = case.N, case.S
    cs, ce = case.cs, case.ce
    ok_q, ok_p = [[int(cs[0]), int(cs[0]) + 1, 0, 0]], [(0, 1)]
    b.profile_reset(); b.profile_enable(1)
    call = lambda pairs=ok_p, q=ok_q, perms=tables, mode=0, other=None: b.restart_overlap_raw(other, pairs, q, perms, mode)
    twice, short = tables.copy(), tables.copy()
    twice[1, 0, 5] = twice[1, 0, 6]
    short[0, 0, S - 1] = S
    bad = [(dict(pairs=[(0, 3)]), 'pair index out of range \\(pair 0\\)'), (dict(pairs=[(0, 1), (-1, 0)]), 'pair index out of range \\(pair 1\\)'),
           (dict(pairs=np.zeros((0, 2), dtype=int)), 'no pairs'),
           (dict(q=[[int(ce[0]), int(ce[0]) + 1, 0, 0]]), 'chain end'), (dict(q=[[int(cs[0]), int(ce[1]), 0, 0]]), 'chain end'),
           (dict(q=[[3, 2, 0, 0]]), 'first <= last'), (dict(q=[[0, N, 0, 0]]), 'first <= last'),
           (dict(q=[[0, 1, len(tables), 0]]), 'permutation index out of range'), (dict(q=[[0, 1, -1, 0]]), 'permutation index out of range'),
           (dict(q=[[0, 1, 0, 1]]), 'field 3'), (dict(q=np.zeros((0, 4), dtype=int)), 'no queries'),
           (dict(perms=twice), 'not a bijection of the states \\(permutation 1\\)'), (dict(perms=short), 'not a bijection of the states \\(permutation 0\\)'),
           (dict(mode=2), 'mode must be'), (dict(mode=-1), 'mode must be')]
    for kw, text in bad:
        with pytest.raises(ValueError, match='^bad argument: restart_overlap: .*' + text):
            call(**kw)
        assert bpmodel.last_error_restarts() == []
    for kw in (dict(pairs=[(0, 1, 2)]), dict(q=[[0, 1, 0]]), dict(perms=tables[:, :, :-1]), dict(perms=tables[0])):
        with pytest.raises(ValueError, match='must have shape'):
            call(**kw)
    # batches of different problems: other segments, and the same problem under another penalty
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=8, num_chains=3, seed=1)
    other = RestartSet(e, synthetic.make_init_params(e, 2, 8), 8, num_clones=3, quiet=True, seeds=[0, 1])
    fresh = _restart_set(*GRIDS[0])
    try:
        other.variational_update(1)
        assert other.batch.num_cn_states == S and other.batch.num_segments != N
        with pytest.raises(ValueError, match='^bad argument: restart_overlap: the two batches describe different problems or devices$'):
            call(other=other.batch)
        # the same problem in a second batch is fine, and a restart of it without update_p_cn is not
        assert np.array_equal(call(other=fresh.batch, pairs=[(0, 1), (2, 2)]), call(pairs=[(0, 1), (2, 2)]))
        fresh.batch.transition_model = 1
        with pytest.raises(ValueError, match='^bad argument: restart_overlap: the two batches describe different problems'):
            call(other=fresh.batch)
    finally:
        other.close(); fresh.close()
    e0 = synthetic.make_experiment(GRIDS[0][0], num_clones=3, max_copy_number=GRIDS[0][2], num_chains=3, seed=0)
    cold = RestartSet(e0, synthetic.make_init_params(e0, 2, GRIDS[0][2]), GRIDS[0][2], num_clones=3, quiet=True, seeds=[0, 1])
    try:
        with pytest.raises(ValueError, match='^restart_overlap before update_p_cn \\(restart 1\\)$') as err:
            call(other=cold.batch, pairs=[(0, 1)])
        assert err.value.restarts == [1]
        with pytest.raises(ValueError, match='update_p_cn'):
            cold.restart_overlap()
    finally:
        cold.close()
    assert b.profile()['k_restart_overlap'][1] == 2; b.profile_enable(0)      # the two good calls above, nothing else
    assert call().shape == (1, 1)
    from oracle import oracle
    oracle.build()
    cpu = RestartSet(e0, synthetic.make_init_params(e0, 2, GRIDS[0][2]), GRIDS[0][2], num_clones=3, quiet=True, seeds=[0, 1], kernel_module=oracle)
    with pytest.raises(NotImplementedError):
        cpu.restart_overlap()


def test_no_side_effects(hip):
    a, c = _restart_set(50, 3, 4, seed=2), _restart_set(50, 3, 4, seed=2)
    try:
        before = [_model_state(m) for m in a.models]
        out = a.restart_overlap([(0, 10), (5, 5), (20, 49)])
        assert out['log_overlap'].shape == (3, 4, 2)
        after = [_model_state(m) for m in a.models]
        for s0, s1 in zip(before, after):
            for k in s0:
                assert np.array_equal(s0[k], s1[k], equal_nan=True), k
        # a fit continued after the call equals one without it
        for rs in (a, c):
            rs.variational_update(2)
        for m1, m2 in zip(a.models, c.models):
            s1, s2 = _model_state(m1), _model_state(m2)
            for k in s1:
                assert np.array_equal(s1[k], s2[k], equal_nan=True), k
        assert np.array_equal(a.calculate_elbo(), c.calculate_elbo())
    finally:
        a.close(); c.close()


def test_clone_order(hip):
    """Two fits from initial parameters that differ only by the order of the tumour clones' h, and a third started at another
    ploidy.  Read state by state the first two disagree; under the map that exchanges the clones they are one solution: the
    distance rate under the swap is the smaller, clone_map picks it, and single linkage at a threshold between the two
    scales joins them and leaves the third apart.

    The threshold was read off this run's printed figures (MI355X).  h after the fit: (0.04, 0.039, 0.021), (0.04, 0.021, 0.039),
    (0.0397, 0.0366, 0.0127).  Distance rate, pairs (0, 1), (0, 2), (1, 2) x [identity, swap]:
        [[6.321260e-01 8.326673e-18]
         [8.110232e-01 9.591273e-01]
         [9.591273e-01 8.110232e-01]]
    and at the best clone map, as a matrix:
        [[0.000000e+00 8.326673e-18 8.110232e-01]
         [8.326673e-18 0.000000e+00 8.110232e-01]
         [8.110232e-01 8.110232e-01 0.000000e+00]]
    The mirrored fits are one solution to rounding; every other figure, the mirrored pair read under the identity included
    (0.63), is above 0.6 per segment.  0.1 lies between the two scales with a factor of six to the nearer one."""
    from remixt_amd.restarts import RestartSet
    e = synthetic.make_experiment(120, num_clones=3, max_copy_number=4, num_chains=3, seed=5)
    p = synthetic.make_init_params(e, 1, 4)[0]
    hn, ht = p['h_normal'], p['h_tumour']
    h = np.array([[hn, 0.65 * ht, 0.35 * ht], [hn, 0.35 * ht, 0.65 * ht], [hn, 0.5 * 0.65 * ht, 0.5 * 0.35 * ht]])
    rs = RestartSet(e, [p, p, p], 4, num_clones=3, quiet=True, seeds=[7, 7, 7], h_init=h)
    try:
        rs.fit(2, 2)
        out = rs.restart_overlap()
        assert [tuple(x) for x in out['pairs']] == [(0, 1), (0, 2), (1, 2)] and out['clone_maps'] == [(0, 1, 2), (0, 2, 1)]
        rate = out['distance_rate']
        best = rate[np.arange(3), out['clone_map']]
        D = posteriors.pair_matrix(out['pairs'], best, 3)
        np.set_printoptions(precision=6, suppress=False, linewidth=200)
        print('h after the fit:\n%s' % np.array([m.model.h for m in rs.models]))
        print('distance rate (pairs x [identity, swap]):\n%s' % rate)
        print('clone_map: %s' % out['clone_map'])
        print('distance rate at the best clone map:\n%s' % D)
        assert rate[0, 1] < rate[0, 0] and out['clone_map'][0] == 1
        assert np.array_equal(best, rate.min(axis=1))
        THRESHOLD = 0.1
        labels = posteriors.cluster_restarts(D, THRESHOLD)
        assert labels.tolist() == [0, 0, 1]
        assert posteriors.cluster_restarts(posteriors.pair_matrix(out['pairs'], rate[:, 0], 3), THRESHOLD).tolist() == [0, 1, 2]
    finally:
        rs.close()
