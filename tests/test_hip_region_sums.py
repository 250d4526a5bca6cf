"""Region sums on the device (rmx_region_sums / k_region_sums): against the log-domain numpy twin on the read-back
framelogprob / log_transmat, the identities that tie a sum to rmx_region_automaton, rmx_region_prob and rmx_region_moments and
a call to one with fewer bins, the sampler, bit-identity of restart ranges, query batches and orders, staging chunks and the
place of the weights in the pool, two state classes, the mixed transition model in both directions, inserted segments, no side
effects on the model, errors, and the public forms at the four class levels."""
import ctypes as C

import numpy as np
import pytest

from remixt_amd import posteriors, restarts, synthetic
from tests import helpers as H
from tests import sums_twin
from tests.test_hip_region_automaton import _close, _inserted, _same
from tests.test_hip_region_events import Case
from tests.test_hip_sample_cn import GRIDS, _fitted, _model_state

pytestmark = pytest.mark.gpu

MASKS = posteriors.MASK_NAMES
BINS = {165: (1, 16, 17, 64), 355: (1, 16, 32), 457: (1, 16, 32)}
TABLES = ('mask', 'total', 'random')
WEIGHTS = ('ones', 'random', 'saturating')


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


def level_tables(cn_classes, seed=0):
    """int16 (C, 3, S): the LOH mask as a 0/1 table, the tumour clones' highest total, and random levels in 0 .. 3."""
    cn = np.asarray(cn_classes)
    rng = np.random.RandomState(91 + seed)
    loh = posteriors.event_tables(cn)[0][:, MASKS.index('loh')] != 0
    total = posteriors._level_quantity(cn, 'total').max(axis=-1)
    return np.ascontiguousarray(np.stack([loh, total, rng.randint(0, 4, size=cn.shape[:2])], axis=1).astype(np.int16))


def run_weights(kind, a, b):
    """The weights of the run [a, b]: all 1; random in 0 .. 5 with zeros; or one that saturates any number of bins (and, times a
    level of 2 or more, 32 bits) among small ones."""
    L = b - a + 1
    rng = np.random.RandomState(1000 * a + b)
    if kind == 'ones':
        return np.ones(L, dtype=np.int64)
    w = rng.randint(0, 6, size=L)
    w[rng.randint(L)] = 0
    if kind == 'saturating':
        w[L // 2] = 2 ** 31 - 1
    return w.astype(np.int64)


class SumsCase(Case):
    def __init__(self, *args, **kw):
        Case.__init__(self, *args, **kw)
        self._want = {}

    def sums(self, runs, levels, combos, bins, r0=None, nr=1, pad=0):
        """(nr, len(runs), len(combos), bins): combos are (level table index, weight kind or a vector per model segment); pad: unused
        weights in front of every run's."""
        q, pool = [], [np.full(pad, 3, dtype=np.int64)]
        at = pad
        for a, b in runs:
            for li, wk in combos:
                w = run_weights(wk, a, b) if isinstance(wk, str) else np.asarray(wk)[a:b + 1]
                q.append([a, b, li, at])
                pool += [w, np.full(pad, 3, dtype=np.int64)]
                at += len(w) + pad
        out = self.b.region_sums_raw(self.r if r0 is None else r0, nr, np.array(q, dtype=np.int32), levels, np.concatenate(pool), bins)
        return out.reshape(nr, len(runs), len(combos), bins)

    def want(self, key, a, b, level_seg, w, bins):
        k = (key, a, b, bins)
        if k not in self._want:
            self._want[k] = sums_twin.logsums(self.twin, a, b, level_seg, [int(x) for x in w], bins)
        return self._want[k]

    def check(self, runs, bins_list, combos, tag='', seed=0):
        """|e^F - e^twin| <= L 1e-9 in every bin; |F - twin| <= L 1e-9 where the twin is >= -300; twin -inf -> -inf exactly;
        -inf only where the twin is -inf or below -700.  Returns (worst error over bound, bins the twin finds unreachable)."""
        worst, unreachable = 0., 0
        levels = level_tables(self.b.cn_classes, seed)
        for bins in bins_list:
            got = self.sums(runs, levels, [(TABLES.index(t), wk) for t, wk in combos], bins)[0]
            for i, (a, b) in enumerate(runs):
                L = b - a + 1
                for j, (t, wk) in enumerate(combos):
                    want = self.want((t, wk, seed), a, b, levels[self.b.seg_class, TABLES.index(t)], run_weights(wk, a, b), bins)
                    g = got[i, j]
                    assert g.shape == (bins,) and not np.isnan(g).any(), (tag, bins, a, b, t, wk, g)
                    err = np.abs(np.exp(g) - np.exp(want))
                    with np.errstate(invalid='ignore'):
                        lerr = np.where(want >= -300, np.abs(g - want), 0.)
                    worst = max(worst, err.max() / (L * 1e-9), lerr.max() / (L * 1e-9))
                    unreachable += int((want == -np.inf).sum())
                    print('%s bins %d run [%d, %d] table %s weights %s: max |P - twin| %.3e, max |F - twin| (twin >= -300) %.3e, lowest finite twin %.1f, sum P - 1 %.2e' % (
                        tag, bins, a, b, t, wk, err.max(), lerr.max(), want[np.isfinite(want)].min(), np.exp(g).sum() - 1))
                    assert (err <= L * 1e-9).all(), (tag, bins, a, b, t, wk, g, want)
                    assert (lerr <= L * 1e-9).all(), (tag, bins, a, b, t, wk, g, want)
                    assert (g[want == -np.inf] == -np.inf).all(), (tag, bins, a, b, t, wk, g, want)
                    assert (want[g == -np.inf] < -700).all(), (tag, bins, a, b, t, wk, g, want)
        print('%s worst error over bound: %.3e; unreachable bins: %d' % (tag, worst, unreachable))
        return worst, unreachable


ALL_COMBOS = [(t, wk) for t in TABLES for wk in WEIGHTS]
DIAGONAL = list(zip(TABLES, WEIGHTS))


@pytest.fixture(scope='module')
def cases(hip):
    made = dict(((N, M, c), SumsCase(_fitted(hip, N, M, c))) for N, M, c in GRIDS)
    yield made
    _close(*[case.m for case in made.values()])


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_twin(hip, cases, N, M, max_cn):
    """Case.queries(): one segment, neighbours over a plain and over a breakend adjacency, the longest chain, a chain start and a
    chain end.  Every table with every weighting: at 1, 16, 17 and 64 bins at 165 states (one, two and four column tiles), at 1,
    16 and 32 bins at 355 and 457 states (8 row tiles per wave)."""
    case = cases[(N, M, max_cn)]
    assert case.S == {8: 165, 12: 355, 6: 457}[max_cn] and case.S % 16
    assert case.m.num_breakpoints > 0 and (case.bidx >= 0).any()
    runs = case.queries()
    c = int(np.argmax(case.ce - case.cs))
    assert (int(case.cs[c]), int(case.ce[c])) in runs and any(a == b for a, b in runs)
    assert posteriors.sums_max_bins(case.S) == max(BINS[case.S])
    worst, unreachable = case.check(runs, BINS[case.S], ALL_COMBOS, tag='S %d' % case.S)
    assert worst <= 1. and unreachable >= 1
    # the model-level form
    levels = level_tables(case.b.cn_classes)
    q = np.array([[a, b, 1, 0] for a, b in runs], dtype=np.int32)
    w = np.ones(max(b - a + 1 for a, b in runs), dtype=np.int32)
    one = case.m.model.region_sums(q, levels, w, 16)
    assert one.shape == (len(q), 16) and np.array_equal(one, case.b.region_sums_raw(case.r, 1, q, levels, w, 16)[0])


@pytest.mark.parametrize('N,M,max_cn,S,bins', [(20, 3, 11, 300, (33, 64)), (16, 3, 15, 544, (17, 32)), (16, 3, 16, 617, (16,))])
def test_the_other_instantiations(hip, N, M, max_cn, S, bins):
    """The instantiations the three grids above do not reach, against the twin: 300 states at 64 bins (8 row tiles per wave, four
    column tiles, the largest LDS plan of that range: 304 rows of 524 bytes), 544 states at 32 bins (16 row tiles, two column
    tiles) and 617 states at 16 bins (16 row tiles, one column tile).  A segment, a pair and the longest chain; each table with one
    weighting, and the copy-number table with the saturating one (a product past 32 bits)."""
    m = _fitted(hip, N, M, max_cn)
    case = SumsCase(m)
    assert case.S == S and posteriors.sums_max_bins(S) == max(bins)
    c = int(np.argmax(case.ce - case.cs))
    a, z = int(case.cs[c]), int(case.ce[c])
    assert z - a >= 3
    worst, unreachable = case.check([(a + 1, a + 1), (a, a + 1), (a, z)], bins, DIAGONAL + [('total', 'saturating')], tag='S %d' % S)
    assert worst <= 1. and unreachable >= 1
    _close(m)


def _counter():
    """The saturating counter automaton: 16 states, delta(q, 1) = min(q + 1, 15), delta(q, 0) = q."""
    return np.array([[[q, min(q + 1, 15)] for q in range(16)]], dtype=np.uint8)


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_identities(hip, cases, N, M, max_cn):
    case = cases[(N, M, max_cn)]
    b, r, con = case.b, case.r, case.constrain
    c = int(np.argmax(case.ce - case.cs))
    seg = np.arange(case.cs[c], case.ce[c] + 1)
    runs = [(int(a), int(z)) for a in seg[::3] for z in seg[::2] if a <= z] + case.queries()
    L = np.array([z - a + 1 for a, z in runs])
    masks = case.masks
    names = ('loh', 'subclonal', 'not_hdel')
    tabs = np.ascontiguousarray(np.stack([masks[:, MASKS.index(k)] for k in names], axis=1).astype(np.int16))
    combos = [(i, con.astype(np.int64)) for i in range(len(names))]
    top = max(BINS[case.S])
    # (i) nothing binds: the probabilities sum to 1.  Budget: L 1e-9
    levels = level_tables(b.cn_classes)
    got = case.sums(runs, levels, [(0, 'ones'), (1, 'random'), (2, 'saturating')], top)[0]
    e = np.abs(np.exp(got).sum(axis=-1) - 1)
    print('S %d: max |sum P - 1| / L %.3e' % (case.S, (e / L[:, None]).max()))
    assert (e <= L[:, None] * 1e-9).all()
    # (ii) weights 1 / 0 = seg_is_original, a mask table, 16 bins: rmx_region_automaton with the saturating counter on the same
    # constrain.  Budget: L 1e-9 each side
    got = case.sums(runs, tabs, combos, 16)[0]
    q = np.array([[a, z, i, 0] for a, z in runs for i in range(len(names))], dtype=np.int32)
    ref = b.region_automaton_raw(r, 1, q, tabs, _counter(), np.array([0]), con)[0].reshape(len(runs), len(names), 16)
    e = np.abs(np.exp(got) - np.exp(ref)).max(axis=-1)
    print('S %d: 16 bins against the counter automaton: max |dP| / L %.3e' % (case.S, (e / L[:, None]).max()))
    assert (e <= 2 * L[:, None] * 1e-9).all()
    # (iii) bin 0: rmx_region_prob's event of the negated mask on the same segments
    neg = {'loh': 'not_loh', 'subclonal': 'not_subclonal', 'not_hdel': 'hdel'}
    q = np.array([[a, z, MASKS.index(neg[k]), -1] for a, z in runs for k in names], dtype=np.int32)
    ref = b.region_logprob_raw(r, 1, q, masks, None, con)[0].reshape(len(runs), len(names))
    for bins in (2, top):
        e = np.abs(np.exp(case.sums(runs, tabs, combos, bins)[0][..., 0]) - np.exp(ref))
        print('S %d: bin 0 of %d against rmx_region_prob of the negated mask: max |dP| / L %.3e' % (case.S, bins, (e / L[:, None]).max()))
        assert (e <= 2 * L[:, None] * 1e-9).all()
    # (iv) where the last bin has no mass, mean and variance of the pmf are rmx_region_moments' of the same weighted feature.
    # Budgets: sum_k k L 1e-9 and sum_k k^2 L 1e-9
    rng = np.random.RandomState(12)
    w = rng.randint(0, 3, size=case.N)
    w[~con] = 0
    short = [(a, z) for a, z in runs if 3 * w[a:z + 1].sum() <= top - 2]
    assert len(short) >= 5
    Ls = np.array([z - a + 1 for a, z in short])
    pmf = np.exp(case.sums(short, levels, [(2, w)], top)[0][:, 0])
    assert (pmf[:, -1] == 0).all()
    k = np.arange(top)
    mean = (pmf * k).sum(axis=-1)
    var = (pmf * k ** 2).sum(axis=-1) - mean ** 2
    qm = np.array([[a, z, 0, 0] for a, z in short], dtype=np.int32)
    mom = b.region_moments_raw(r, 1, qm, levels[:, 2:3].astype(float), w[None].astype(float), 1)[0]
    e1, e2 = np.abs(mean - mom[:, 0]), np.abs(var - mom[:, 1])
    b1, b2 = k.sum() * Ls * 1e-9, (k ** 2).sum() * Ls * 1e-9
    print('S %d: mean and variance against rmx_region_moments: max error over budget %.3e, %.3e' % (case.S, (e1 / b1).max(), (e2 / b2).max()))
    assert (e1 <= b1).all() and (e2 <= b2).all()
    # (v) a call with fewer bins: bins 0 .. B' - 2 agree within 2 L 1e-9 and bin B' - 1 is the sum of the rest
    wide = np.exp(case.sums(runs, levels, [(1, 'random'), (2, 'ones')], top)[0])
    for fewer in (1, 2, 7, 16):
        few = np.exp(case.sums(runs, levels, [(1, 'random'), (2, 'ones')], fewer)[0])
        e = np.abs(few[..., :-1] - wide[..., :fewer - 1]).max(axis=-1) if fewer > 1 else np.zeros(few.shape[:2])
        et = np.abs(few[..., -1] - wide[..., fewer - 1:].sum(axis=-1))
        print('S %d: %d bins against %d: max |dP| / L %.3e, last bin %.3e' % (case.S, fewer, top, (e / L[:, None]).max(), (et / L[:, None]).max()))
        assert (e <= 2 * L[:, None] * 1e-9).all() and (et <= (top - fewer + 2) * L[:, None] * 1e-9).all()


def test_against_the_sampler(hip):
    """event_occupancy by segments for 'loh' and 'subclonal' and by length for a gain mask against 4 096 posterior samples (seed 99)
    with the sums formed on the host: every bin within 5 sqrt(p (1 - p) / 4096) + 1e-9 of the exact p."""
    from tests.test_hip_posterior_summary import _fitted as fitted_masked
    m = fitted_masked(hip, 30, 3, 8, sweeps=3, masked=True)
    NS = 4096
    b, r = m.model._batch, m.model._r
    st = b.sample_states(r, 1, NS, [99]).astype(np.int64)[0]                      # (NS, N1)
    cn = b.cn_classes
    orig = np.asarray(m.seg_is_original, dtype=bool)
    fwd, rev = np.asarray(m.seg_fwd_remap), np.asarray(m.seg_rev_remap)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    c = int(np.argmax(ce - cs))
    real = np.flatnonzero(orig)
    runs = [(int(cs[c]), int(ce[c])), (int(cs[c]) + 1, int(cs[c]) + 4), (int(ce[0]), int(ce[0]))]       # (the automaton test's three runs,
    runs = [(int(real[real >= a][0]), int(real[real <= z][-1])) for a, z in runs]                        # from and to a real segment)
    regions = [(int(rev[a]), int(rev[z])) for a, z in runs]
    assert all(fwd[i] == a and fwd[j] == z for (i, j), (a, z) in zip(regions, runs))
    gain = posteriors.level_mask(cn, 'total', 'any', 3, 99)
    informative = 0
    for event, weights in (('loh', 'segments'), ('subclonal', 'segments'), (gain, 'length')):
        out = m.event_occupancy(regions, event, weights=weights, bins=16)
        table = posteriors._event_table(cn, event)
        for i, (a, z) in enumerate(runs):
            held = np.stack([table[b.seg_class[n]][st[:, n]] for n in range(a, z + 1)], axis=1)        # (NS, L)
            real = orig[a:z + 1]
            for side in ('floor', 'ceil'):
                if weights == 'segments':
                    w = real.astype(np.int64)
                else:
                    w = posteriors.quantise_lengths(np.where(real, np.asarray(m.l1)[a:z + 1], 0.), 16, 1, out['unit'][i])[1 if side == 'floor' else 2]
                P = out['pmf_' + side][i]
                freq = np.bincount(np.minimum((held * w).sum(axis=1), 15), minlength=16) / NS
                tol = 5 * np.sqrt(P * (1 - P) / NS) + 1e-9
                print('run [%d, %d] %s %s: exact %s sampled %s' % (a, z, event if isinstance(event, str) else 'gain', side, np.array2string(P, precision=4), np.array2string(freq, precision=4)))
                informative += int(((P > 0.01) & (P < 0.99)).sum()) if side == 'floor' else 0
                assert (np.abs(freq - P) <= tol).all(), (a, z, event, side, freq, P)
    print('informative (run, bin) entries: %d' % informative)
    assert informative >= 3
    _close(m)


def test_bit_identity(hip, cases):
    """A (restart, query) result depends on neither the batch of queries, their order, nor on where its weights lie in the pool."""
    for grid in GRIDS[:2]:
        case = cases[grid]
        runs = case.queries()
        levels = level_tables(case.b.cn_classes)
        combos = [(0, 'ones'), (1, 'random'), (2, 'saturating'), (2, 'ones')]
        for bins in (16, max(BINS[case.S])):
            full = case.sums(runs, levels, combos, bins)[0]
            for i in range(len(runs)):
                assert np.array_equal(case.sums(runs[i:i + 1], levels, combos, bins)[0, 0], full[i]), i
            assert np.array_equal(case.sums(runs[::-1], levels, combos, bins)[0], full[::-1])
            assert np.array_equal(case.sums(runs, levels, combos[::-1], bins)[0], full[:, ::-1])
            assert np.array_equal(case.sums(runs, levels, combos, bins, pad=37)[0], full)             # the weights elsewhere in the pool
            # a level table among several
            more = np.concatenate([np.zeros_like(levels), levels], axis=1)
            assert np.array_equal(case.sums(runs, more, [(li + 3, wk) for li, wk in combos], bins)[0], full)


def test_restart_ranges_and_staging_chunks(hip):
    """Four restarts: a call over 0 .. 3 equals the single-restart calls bit for bit; a call with more queries than the 64 MiB
    staging buffer holds for four restarts of 64 bins runs in two chunks and repeats the short call's numbers."""
    from tests.test_hip_query_driver import _restart_set
    rs = _restart_set(4)
    try:
        b = rs.batch
        case = SumsCase(rs.models[0])
        runs = case.queries()
        levels = level_tables(b.cn_classes)
        combos = [(0, 'ones'), (1, 'random'), (2, 'saturating')]
        call = lambda r0, nr: case.sums(runs, levels, combos, 64, r0=r0, nr=nr)
        full = call(0, 4)
        assert full.shape == (4, len(runs), 3, 64) and not np.isnan(full).any() and len(np.unique(full.reshape(4, -1), axis=0)) > 1
        for r in range(4):
            assert np.array_equal(call(r, 1)[0], full[r]), r
        assert np.array_equal(call(1, 2), full[1:3]) and np.array_equal(call(1, 3), full[1:])
        chunk = (64 << 20) // (4 * 64 * 8 + 16)
        a, z = [(a, z) for a, z in runs if z - a == 1][0]
        base = np.array([[a, z, li, 2 * li] for li in range(3)], dtype=np.int32)
        w = np.array([1, 2, 0, 3, 2 ** 31 - 1, 1], dtype=np.int64)
        reps = chunk // len(base) + 1
        assert reps * len(base) > chunk
        big = b.region_sums_raw(0, 4, np.tile(base, (reps, 1)), levels, w, 64)
        small = b.region_sums_raw(0, 4, base, levels, w, 64)
        assert np.array_equal(big.reshape(4, reps, len(base), 64), np.broadcast_to(small[:, None], (4, reps, len(base), 64)))
    finally:
        rs.close()


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
        case = SumsCase(m, batch=b, r=0)
        levels = level_tables(classes)
        assert not np.array_equal(levels[0, 1], levels[1, 1]) and not np.array_equal(levels[0, 2], levels[1, 2])      # the level tables differ per class
        worst, _ = case.check(case.queries(), (16, 64), ALL_COMBOS, tag='two classes')
        assert worst <= 1.
        # clone 1's total is >= 2 under class 1 and can be 0 under class 0: the level "clone 1's total" of one odd segment is never
        # below 2 (a kernel that took class 0's levels everywhere would put mass there), that of an even one can be
        tot = posteriors._level_quantity(classes, 'total')[:, :, 0].astype(np.int16)[:, None, :]
        assert tot[0].min() == 0 and tot[1].min() == 2
        odd = [(n, n) for n in range(1, N, 2)]
        even = [(n, n) for n in range(0, N, 2)]
        assert (case.sums(odd, tot, [(0, 'ones')], 16)[0, :, 0, :2] == -np.inf).all()
        assert np.isfinite(case.sums(even, tot, [(0, 'ones')], 16)[0, :, 0, :2]).any()
    finally:
        b.close()


def test_mixed_transition_model(hip):
    """The snapshot of the last update_p_cn under another transition_model than the current one, both directions."""
    m = _fitted(hip, 40, 3, 4, seed=3)
    T0 = np.array(m.model.log_transmat)
    m.model.transition_model = 1
    assert np.array_equal(np.array(m.model.log_transmat), T0)            # the snapshot stays the model-0 one
    case = SumsCase(m)
    worst, _ = case.check(case.queries(), (16, 64), DIAGONAL, tag='mixed model 0 -> 1')
    assert worst <= 1.
    m2 = _fitted(hip, 40, 3, 4, seed=3, transition_model=1)
    assert m2.model.transition_model == 1
    m2.model.transition_model = 0
    case2 = SumsCase(m2)
    assert not np.array_equal(np.array(m2.model.log_transmat), T0)
    worst, _ = case2.check(case2.queries(), (16, 64), DIAGONAL, tag='mixed model 1 -> 0')
    assert worst <= 1.
    _close(m, m2)


def test_inserted_segments(hip):
    """Two breakends on one boundary: the model inserts a zero-length segment there.  With weight 0 it does not count, with
    weight 1 it does."""
    m = _inserted(hip)
    case = SumsCase(m)
    assert m.N1 > m.N and not case.constrain.all()
    dummy = int(np.flatnonzero(~case.constrain & (np.arange(m.N1) > 0) & (case.tel == 0))[0])
    assert case.constrain[dummy - 1] and case.constrain[dummy + 1]
    runs = [(dummy - 1, dummy + 1), (dummy, dummy), (dummy, dummy + 1), (dummy - 1, dummy), (dummy - 3, dummy + 2)]
    worst, _ = case.check(runs, (5, 64), ALL_COMBOS, tag='inserted segment')
    assert worst <= 1.
    # a level of 1 everywhere counts the weights: the inserted segment counts under weight 1 and does not under weight 0
    one = np.ones(case.b.cn_classes.shape[:2], dtype=np.int16)[:, None, :]
    for w, first in ((case.constrain.astype(np.int64), [2, 0, 1, 1]), (np.ones(m.N1, dtype=np.int64), [3, 1, 2, 2])):
        want = first + [int(w[dummy - 3:dummy + 3].sum())]
        got = case.sums(runs, one, [(0, w)], 8)[0, :, 0]
        assert np.array_equal(np.argmax(got, axis=-1), want) and (np.abs(got.max(axis=-1)) <= 6e-9).all() and ((got == -np.inf).sum(axis=-1) == 7).all(), (w, got)
    # the subclonal segments of the experiment pair around it, through event_occupancy: the twin on the model run, the inserted segment at weight 0
    i = int(m.seg_rev_remap[dummy - 1])
    assert m.seg_fwd_remap[i] == dummy - 1 and m.seg_fwd_remap[i + 1] == dummy + 1
    out = m.event_occupancy([(i, i + 1)], 'subclonal', weights='segments', bins=4)
    ev = posteriors._event_table(case.b.cn_classes, 'subclonal').astype(int)[case.b.seg_class]
    want = np.exp(sums_twin.logsums(case.twin, dummy - 1, dummy + 1, ev, [1, 0, 1], 4))
    assert out['pmf_floor'].shape == (1, 4) and np.abs(out['pmf_floor'][0] - want).max() <= 3e-9 and out['pmf_floor'][0, 3] == 0 and out['exact'][0]
    _close(m)


def test_no_side_effects(hip):
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    before = _model_state(m1)
    out = m1.event_occupancy([(0, 10), (5, 5), (3, 12)], 'loh')
    seg = m1.event_occupancy([(0, 10), (5, 5)], ('total', 1), weights='segments', bins=64)
    assert out['pmf_floor'].shape == (3, 64) and out['pmf_ceil'].shape == (3, 64) and seg['pmf_floor'].shape == (2, 64) and seg['exact'].all()
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
    levels = level_tables(b.cn_classes)
    w = np.array([1, 2, 0, 3], dtype=np.int32)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    ok = [[int(cs[0]), int(cs[0]) + 1, 0, 1]]
    with pytest.raises(ValueError, match='update_p_cn'):
        b.region_sums_raw(r, 1, ok, levels, w, 8)
    assert bpmodel.last_error_restarts() == [r]
    with pytest.raises(ValueError, match='update_p_cn'):
        m.event_occupancy([(0, 3)], 'loh')
    m.variational_update()
    N = b.num_segments
    lib, handle = b._lib, b._handle
    dp, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert b.region_sums_raw(r, 1, ok, levels, w, 8).shape == (1, 1, 8)
    neg_levels = levels.copy(); neg_levels[-1, -1, -1] = -1
    # (queries, levels, weights, bins, words of the message)
    bad = [(ok, levels, w, 0, 'nbins'), (ok, levels, w, 65, 'nbins'), (ok, levels, w, -1, 'nbins'),
           (ok, neg_levels, w, 8, 'level entry is negative'), (ok, levels, np.array([1, 2, -1, 3]), 8, 'weight is negative'),
           (ok + [[0, 1, -1, 0]], levels, w, 8, 'level table index'), (ok + [[0, 1, 3, 0]], levels, w, 8, 'level table index'),
           (ok + [[0, 1, 0, -1]], levels, w, 8, 'weight offset'), (ok + [[0, 1, 0, 4]], levels, w, 8, 'weight offset'),
           (ok + [[0, 1, 0, 3]], levels, w, 8, 'leave the pool'), (ok + [[0, 2, 0, 2]], levels, w, 8, 'leave the pool'),
           (ok + [[3, 2, 0, 0]], levels, w, 8, 'first <= last'), (ok + [[int(ce[0]), int(ce[0]) + 1, 0, 0]], levels, w, 8, 'chain end'),
           (ok + [[0, N, 0, 0]], levels, w, 8, 'first <= last'), (ok + [[-1, 0, 0, 0]], levels, w, 8, 'first <= last')]
    for q, lv, wt, bins, text in bad:
        # through the C entry point with an output buffer of its own: refused, and the buffer is untouched
        qa, args, _keep = b._region_args(q, None, lv, None)
        wt = np.ascontiguousarray(wt, dtype=np.int32)
        obuf = np.full((len(q), 64), 7.25)
        rc = lib.rmx_region_sums(handle, r, 1, args[0], args[1], args[4], args[5], len(wt), wt.ctypes.data_as(i32p), bins, obuf.ctypes.data_as(dp))
        assert rc == 5 and (obuf == 7.25).all(), (q, text, rc)
        with pytest.raises(ValueError, match='^bad argument: .*' + text):
            b.region_sums_raw(r, 1, q, lv, wt, bins)
        assert bpmodel.last_error_restarts() == []
    qa, args, _keep = b._region_args(ok, None, levels, None)
    obuf = np.full((2, 1, 8), 7.25)
    out = obuf.ctypes.data_as(dp)
    wp = w.ctypes.data_as(i32p)
    call = lambda r0=r, nr=1, nq=args[0], qp=args[1], nlevel=args[4], lp=args[5], nwt=4, wtp=wp, o=out: lib.rmx_region_sums(
        handle, r0, nr, nq, qp, nlevel, lp, nwt, wtp, 8, o)
    for r0, nr in ((-1, 1), (0, 0), (0, 2)):
        assert call(r0=r0, nr=nr) == 5
    # nq < 1, NULL pointers, nlevel < 1, nwt < 1
    assert call(nq=0) == 5 and call(qp=None) == 5 and call(lp=None) == 5 and call(nlevel=0) == 5 and call(wtp=None) == 5 and call(nwt=0) == 5 and call(o=None) == 5
    assert (obuf == 7.25).all()
    assert call() == 0 and not (obuf[0] == 7.25).any() and (obuf[1] == 7.25).all()
    for kw in (dict(event='loh', bins=65), dict(event='gain'), dict(event='loh', weights='area')):
        with pytest.raises(ValueError):
            m.event_occupancy([(0, 3)], **kw)
    _close(m)


def test_more_bins_than_the_state_count_holds(hip, cases):
    """64 bins at 355 states: RMX_EUNSUPPORTED from an argument check, nothing launched, the output untouched; 32 are fine."""
    case = cases[GRIDS[1]]
    b, r = case.b, case.r
    assert case.S == 355
    levels = level_tables(b.cn_classes)
    a, z = case.queries()[1]
    q, args, _keep = b._region_args([[a, z, 0, 0]], None, levels, None)
    w = np.ones(2, dtype=np.int32)
    obuf = np.full((1, 64), 7.25)
    rc = b._lib.rmx_region_sums(b._handle, r, 1, args[0], args[1], args[4], args[5], 2, w.ctypes.data_as(C.POINTER(C.c_int32)), 64, obuf.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 4 and (obuf == 7.25).all()
    with pytest.raises(NotImplementedError, match='at most 32 bins'):
        b.region_sums_raw(r, 1, q, levels, w, 64)
    with pytest.raises(ValueError, match='at most 32 bins'):
        case.m.event_occupancy([(0, 3)], 'loh', bins=64)
    assert b.region_sums_raw(r, 1, q, levels, w, 32).shape == (1, 1, 32)
    assert case.m.event_occupancy([(0, 3)], 'loh')['bins'] == 32


REGIONS = [(2, 7), (17, 17), (10, 30), (0, 39), (12, 13)]


def _examples(cn, num_model_segments, orig):
    gain = posteriors.level_mask(cn, 'total', 'any', 3, 99)
    w = np.where(orig, np.arange(num_model_segments) % 3, 0)
    return {'event_occupancy': [dict(regions=REGIONS, event='loh'), dict(regions=REGIONS, event=gain, weights='segments', bins=16),
                                dict(regions=REGIONS, event=('total', 1), weights='length', bins=32, unit=None)],
            'region_sums': [dict(regions=REGIONS, levels=posteriors._level_quantity(cn, 'total')[:, :, 0], weights=w, bins=24)]}


def _direct(name, b, r0, nr, m, a):
    maps = (m.seg_fwd_remap, m.seg_is_original, m.is_telomere)
    if name == 'event_occupancy':
        return posteriors.batch_event_occupancy(b, r0, nr, a['regions'], *maps, m.l1, a['event'], weights=a.get('weights', 'length'), bins=a.get('bins'), unit=a.get('unit'))
    return posteriors.batch_region_sums(b, r0, nr, a['regions'], *maps, levels=a['levels'], weights=a['weights'], bins=a['bins'])


def _strip(entry, out):
    return dict((key, v if key in entry.shared else v[0]) for key, v in out.items())


def test_the_four_class_levels(hip):
    """Every level returns the numbers of the posteriors.batch_* function called directly, which asks the raw call; event_occupancy
    by segments of a region in one chain is the raw call's distribution."""
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
        assert chain[2] == chain[7] and chain[10] != chain[30] and chain[0] != chain[39] and chain[12] != chain[13]      # (REGIONS has regions in two and in three chains)
        orig = np.asarray(models[0].seg_is_original, dtype=bool)
        examples = _examples(b.cn_classes, b.num_segments, orig)
        set_answers = {}
        for name, given_list in examples.items():
            entry = queries.entry(name)
            for k, given in enumerate(given_list):
                want = _direct(name, b, 0, R, models[0], given)
                got = getattr(rs, name)(**given)
                _same(got, want, 'set: %s %d' % (name, k))
                set_answers[(name, k)] = got
                for r, m in enumerate(models):
                    _same(getattr(m, name)(**given), _strip(entry, _direct(name, b, r, 1, m, given)), 'model %d: %s %d' % (r, name, k))
        # against the raw call: a region inside one chain is one query
        fwd = np.asarray(models[0].seg_fwd_remap)
        gain = posteriors.level_mask(b.cn_classes, 'total', 'any', 3, 99)
        q = np.array([[fwd[2], fwd[7], 0, 0]], dtype=np.int32)
        raw = b.region_sums_raw(0, R, q, gain.astype(np.int16)[:, None, :], orig[fwd[2]:fwd[7] + 1].astype(np.int32), 16)
        occ = set_answers[('event_occupancy', 1)]
        assert np.abs(occ['pmf_floor'][:, 0] - np.exp(raw[:, 0])).max() <= 1e-15 and occ['exact'].all() and np.array_equal(occ['pmf_floor'], occ['pmf_ceil'])
        assert np.array_equal(occ['length'], [6, 1, 21, 40, 2]) and np.abs(occ['pmf_floor'].sum(axis=-1) - 1).max() <= 1e-7
        lo, hi = posteriors.occupancy_at_least(set_answers[('event_occupancy', 0)], 0.5)
        assert lo.shape == (R, len(REGIONS)) and (lo <= hi + 1e-15).all()
    finally:
        rs.close()
    g = restarts.RestartGroups(e, ps, MAX_CN, groups=2, num_clones=3, quiet=True, seeds=list(range(R)), options={'fb_nv': 1})
    try:
        g.variational_update(2)
        g.synchronize()
        for name, given_list in examples.items():
            entry = queries.entry(name)
            for k, given in enumerate(given_list):
                parts = [getattr(part, name)(**given) for part in g.sets]
                got = getattr(g, name)(**given)
                _same(got, restarts._join(parts, shared=entry.shared), 'groups: %s %d' % (name, k))
                for key in got:
                    assert np.shape(got[key]) == np.shape(set_answers[(name, k)][key])
    finally:
        g.close()
    dg = restarts.DatasetGroups([e, e], [ps[:2], ps[2:]], MAX_CN, seeds=[[0, 1], [2, 3]], num_clones=3, quiet=True, options={'fb_nv': 1})
    try:
        dg.variational_update(2)
        dg.synchronize()
        for name, given_list in examples.items():
            for k, given in enumerate(given_list):
                want = [getattr(part, name)(**given) for part in dg.parts]
                got = getattr(dg, name)(**given)
                assert len(got) == 2
                for d in range(2):
                    _same(got[d], want[d], 'datasets: %s %d' % (name, k))
    finally:
        dg.close()
