"""Region automata on the device (rmx_region_automaton / k_region_automaton): against the log-domain numpy twin on the read-back
framelogprob / log_transmat, the identities that tie an automaton to rmx_region_prob, rmx_region_extremes and
rmx_region_pattern, the sampler, bit-identity of restart ranges, query batches and orders, staging chunks and padding with
unreachable states, two state classes, the mixed transition model in both directions, inserted segments, no side effects on
the model, errors, and the public forms at the four class levels.

A crafted zero normaliser is left out: the siblings' tests show no way to make D(s') zero under positive mass that does not
go through set_array on the forward plane of a live batch, which none of them does."""
import ctypes as C

import numpy as np
import pytest

from remixt_amd import posteriors, restarts, synthetic
from tests import automaton_twin
from tests import helpers as H
from tests.test_hip_region_events import Case
from tests.test_hip_sample_cn import GRIDS, _fitted, _model_state

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (5, 2), (16, 16))
MASKS = posteriors.MASK_NAMES


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


def automata(Q, A, seed=0):
    """(delta (3, Q, A), start (3,)): a random delta, a permutation delta (every symbol permutes the states), and a delta that
    sends every state to one."""
    rng = np.random.RandomState(1000 * Q + A + seed)
    rand = rng.randint(0, Q, size=(Q, A))
    perm = np.stack([rng.permutation(Q) for _ in range(A)], axis=1)
    one = np.full((Q, A), Q // 2)
    return np.stack([rand, perm, one]).astype(np.uint8), np.array([0, Q - 1, Q // 3], dtype=np.int32)


def symbol_tables(cn_classes, A, seed=0):
    """int16 (C, 3, S) with entries in [0, A): the tumour clones' highest total, random symbols, and hdel / loh / subclonal."""
    cn = np.asarray(cn_classes)
    rng = np.random.RandomState(77 + A + seed)
    total = np.clip(posteriors._level_quantity(cn, 'total').max(axis=-1), 0, A - 1)
    events = np.clip(posteriors.symbols_from(cn, ['hdel', 'loh', 'subclonal']), 0, A - 1)
    return np.ascontiguousarray(np.stack([total, rng.randint(0, A, size=cn.shape[:2]), events], axis=1).astype(np.int16))


class AutomatonCase(Case):
    def __init__(self, *args, **kw):
        Case.__init__(self, *args, **kw)
        self._want = {}

    def final(self, runs, sym, delta, start, combos, constrain='case', r0=None, nr=1):
        """(nr, len(runs), len(combos), Q): combos are (symbol table, automaton) index pairs."""
        q = np.array([[a, b, si, ui] for (a, b) in runs for (si, ui) in combos], dtype=np.int32)
        con = self.constrain if isinstance(constrain, str) else constrain
        out = self.b.region_automaton_raw(self.r if r0 is None else r0, nr, q, sym, delta, start, con)
        return out.reshape(nr, len(runs), len(combos), delta.shape[1])

    def want(self, key, a, b, sym_seg, delta, start, constrain):
        k = (key, a, b)
        if k not in self._want:
            self._want[k] = automaton_twin.logfinal(self.twin, a, b, sym_seg, delta, start, constrain)
        return self._want[k]

    def check(self, runs, shapes=SHAPES, combos=((0, 0), (1, 1), (2, 2)), constrain='case', tag='', seed=0):
        """|e^F - e^twin| <= L 1e-9 in every column; |F - twin| <= L 1e-9 where the twin is >= -300; twin -inf -> -inf exactly;
        -inf only where the twin is -inf or below -700.  Returns (worst error over bound, columns the twin finds unreachable)."""
        worst, unreachable = 0., 0
        con = self.constrain if isinstance(constrain, str) else constrain
        for Q, A in shapes:
            delta, start = automata(Q, A, seed)
            sym = symbol_tables(self.b.cn_classes, A, seed)
            got = self.final(runs, sym, delta, start, combos, constrain=con)[0]
            for i, (a, b) in enumerate(runs):
                L = b - a + 1
                for j, (si, ui) in enumerate(combos):
                    want = self.want((Q, A, si, ui, seed, None if con is None else con.tobytes()), a, b, sym[self.b.seg_class, si], delta[ui], start[ui], con)
                    g = got[i, j]
                    assert g.shape == (Q,) and not np.isnan(g).any(), (tag, Q, A, a, b, si, ui, g)
                    err = np.abs(np.exp(g) - np.exp(want))
                    with np.errstate(invalid='ignore'):
                        lerr = np.where(want >= -300, np.abs(g - want), 0.)
                    worst = max(worst, err.max() / (L * 1e-9), lerr.max() / (L * 1e-9))
                    unreachable += int((want == -np.inf).sum())
                    print('%s Q %d A %d run [%d, %d] symbols %d automaton %d: max |P - twin| %.3e, max |F - twin| (twin >= -300) %.3e, lowest finite twin %.1f, sum P - 1 %.2e' % (
                        tag, Q, A, a, b, si, ui, err.max(), lerr.max(), want[np.isfinite(want)].min(), np.exp(g).sum() - 1))
                    assert (err <= L * 1e-9).all(), (tag, Q, A, a, b, si, ui, g, want)
                    assert (lerr <= L * 1e-9).all(), (tag, Q, A, a, b, si, ui, g, want)
                    assert (g[want == -np.inf] == -np.inf).all(), (tag, Q, A, a, b, si, ui, g, want)
                    assert (want[g == -np.inf] < -700).all(), (tag, Q, A, a, b, si, ui, g, want)
        print('%s worst error over bound: %.3e; unreachable columns: %d' % (tag, worst, unreachable))
        return worst, unreachable


def _close(*models):
    """The device batches of fitted models, given back now and not whenever the collector finds them."""
    for m in models:
        m.model._batch.close()


@pytest.fixture(scope='module')
def cases(hip):
    made = dict(((N, M, c), AutomatonCase(_fitted(hip, N, M, c))) for N, M, c in GRIDS)
    yield made
    _close(*[case.m for case in made.values()])


@pytest.mark.parametrize('N,M,max_cn', GRIDS)
def test_against_twin(hip, cases, N, M, max_cn):
    """Case.queries(): one segment, neighbours over a plain and over a breakend adjacency, the longest chain, a chain start and a
    chain end; three shapes with a random, a permutation and a collapsing delta each."""
    case = cases[(N, M, max_cn)]
    assert case.S == {8: 165, 12: 355, 6: 457}[max_cn] and case.S % 16
    assert case.m.num_breakpoints > 0 and (case.bidx >= 0).any()
    runs = case.queries()
    c = int(np.argmax(case.ce - case.cs))
    assert (int(case.cs[c]), int(case.ce[c])) in runs and any(a == b for a, b in runs)
    worst, unreachable = case.check(runs, tag='S %d' % case.S)
    assert worst <= 1. and unreachable >= 1
    # the model-level form
    delta, start = automata(5, 2)
    sym = symbol_tables(case.b.cn_classes, 2)
    q = np.array([[a, b, 0, 1] for a, b in runs], dtype=np.int32)
    one = case.m.model.region_automaton(q, sym, delta, start, case.constrain)
    assert one.shape == (len(q), 5) and np.array_equal(one, case.b.region_automaton_raw(case.r, 1, q, sym, delta, start, case.constrain)[0])


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
    sym = np.ascontiguousarray(np.stack([masks[:, MASKS.index(k)] for k in names], axis=1).astype(np.int16))
    combos = [(i, 0) for i in range(len(names))]
    # (i) nothing binds: the Q probabilities sum to 1.  Budget: L 1e-9
    delta, start = automata(16, 16)
    got = case.final(runs, symbol_tables(b.cn_classes, 16), delta, start, [(0, 0), (1, 1), (2, 2)])[0]
    e = np.abs(np.exp(got).sum(axis=-1) - 1)
    print('S %d: max |sum P - 1| / L %.3e' % (case.S, (e / L[:, None]).max()))
    assert (e <= L[:, None] * 1e-9).all()
    # (ii) the two-state trap automaton: state 0 = every read segment was in the mask.  Column 0 is rmx_region_prob's event with the
    # same mask and constrain.  Budget: L 1e-9 each side
    trap = np.array([[[1, 0], [1, 1]]], dtype=np.uint8)
    got = case.final(runs, sym, trap, np.array([0]), combos)[0]
    q = np.array([[a, z, MASKS.index(k), -1] for a, z in runs for k in names], dtype=np.int32)
    ref = b.region_logprob_raw(r, 1, q, masks, None, con)[0].reshape(len(runs), len(names))
    e = np.abs(np.exp(got[..., 0]) - np.exp(ref))
    print('S %d: trap automaton against rmx_region_prob: max |dP| / L %.3e' % (case.S, (e / L[:, None]).max()))
    assert (e <= 2 * L[:, None] * 1e-9).all()
    # (iv) automaton_runs: no run at all is rmx_region_prob's event of the negated mask
    au = posteriors.automaton_runs(8)
    runs8 = case.final(runs, sym, au.delta[None], np.array([au.start]), combos)[0]
    pmf = np.exp(runs8).reshape(len(runs), len(names), 8, 2).sum(axis=-1)
    neg = {'loh': 'not_loh', 'subclonal': 'not_subclonal', 'not_hdel': 'hdel'}
    q = np.array([[a, z, MASKS.index(neg[k]), -1] for a, z in runs for k in names], dtype=np.int32)
    ref = b.region_logprob_raw(r, 1, q, masks, None, con)[0].reshape(len(runs), len(names))
    e = np.abs(pmf[..., 0] - np.exp(ref))
    print('S %d: automaton_runs bin 0 against rmx_region_prob of the negated mask: max |dP| / L %.3e' % (case.S, (e / L[:, None]).max()))
    assert (e <= 2 * L[:, None] * 1e-9).all()
    # (iii) the running-maximum automaton: delta(q, x) = max(q, x) over the tumour clones' highest total.  Its cdf is
    # rmx_region_extremes' columns.  Budget: (j + 1) L 1e-9 for the sum of j + 1 columns, L 1e-9 for the other side
    levels, lnames = posteriors.level_tables(b.cn_classes, 16)
    li = lnames.index('peak_total_any')
    peak = np.maximum(np.arange(16)[:, None], np.arange(16)[None, :]).astype(np.uint8)
    got = case.final(runs, np.ascontiguousarray(levels[:, li:li + 1]), peak[None], np.array([0]), [(0, 0)])[0, :, 0]
    q = np.array([[a, z, -1, li] for a, z in runs], dtype=np.int32)
    ref = b.region_extremes_raw(r, 1, q, None, levels, con, 16)[0]
    e = np.abs(np.cumsum(np.exp(got), axis=-1) - np.exp(ref))
    print('S %d: running maximum against rmx_region_extremes: max |d cdf| / L %.3e' % (case.S, (e / L[:, None]).max()))
    assert (e <= (np.arange(16)[None, :] + 2) * L[:, None] * 1e-9).all()
    # (v) the mean number of runs, where the last bin cannot saturate (at most 7 runs in 14 segments): every run starts once, at a or
    # behind a segment outside the mask.  Every segment is read (constrain = None on both sides).  Budgets: sum_k k L 1e-9 = 28 L 1e-9
    # for the mean of the pmf; 1e-9 for the one-segment query and 2e-9 for each of the L - 1 two-segment patterns
    short = [(a, z) for a, z in runs if z - a + 1 <= 14]
    Ls = np.array([z - a + 1 for a, z in short])
    runs8 = case.final(short, sym, au.delta[None], np.array([au.start]), combos, constrain=None)[0]
    mean = (np.exp(runs8).reshape(len(short), len(names), 8, 2).sum(axis=-1) * np.arange(8)).sum(axis=-1)
    for j, k in enumerate(names):
        mi, ni = MASKS.index(k), MASKS.index(neg[k])
        first = np.exp(b.region_logprob_raw(r, 1, np.array([[a, a, mi, -1] for a, z in short], dtype=np.int32), masks, None, None)[0])
        pieces = np.array([[x, x, m_, -1] for a, z in short for n in range(a, z) for x, m_ in ((n, ni), (n + 1, mi))], dtype=np.int32).reshape(-1, 4)
        want = first.copy()
        if len(pieces):
            qq = np.array([[2 * i, 2, 0, 0] for i in range(len(pieces) // 2)], dtype=np.int32)
            begins = np.exp(b.region_pattern_raw(r, 1, qq, pieces, masks, None, None)[0])
            owner = np.repeat(np.arange(len(short)), [z - a for a, z in short])
            np.add.at(want, owner, begins)
        e = np.abs(mean[:, j] - want)
        print('S %d: mean number of %s runs against rmx_region_pattern: max error over budget %.3e' % (case.S, k, (e / ((28 * Ls + 1 + 2 * (Ls - 1)) * 1e-9)).max()))
        assert (e <= (28 * Ls + 1 + 2 * (Ls - 1)) * 1e-9).all(), k


def test_against_the_sampler(hip):
    """The final-state distribution of automaton_runs(4), automaton_run_of(2) and automaton_switches(3) against 4 096 posterior
    samples (seed 99) with the automaton run on the host: every column within 5 sqrt(p (1 - p) / 4096) + 1e-9 of the exact p."""
    from tests.test_hip_posterior_summary import _fitted as fitted_masked
    m = fitted_masked(hip, 30, 3, 8, sweeps=3, masked=True)
    NS = 4096
    b, r = m.model._batch, m.model._r
    st = b.sample_states(r, 1, NS, [99]).astype(np.int64)[0]                      # (NS, N1)
    cn = b.cn_classes
    orig = np.asarray(m.seg_is_original, dtype=bool)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    c = int(np.argmax(ce - cs))
    runs = [(int(cs[c]), int(ce[c])), (int(cs[c]) + 1, int(cs[c]) + 4), (int(ce[0]), int(ce[0]))]
    two = posteriors.symbols_from(cn, [posteriors.level_mask(cn, 'total', 'any', 0, 2), posteriors.level_mask(cn, 'total', 'any', 3, 99)])
    informative = 0
    for au, sym in ((posteriors.automaton_runs(4), posteriors.symbols_from(cn, ['loh'])), (posteriors.automaton_run_of(2), posteriors.symbols_from(cn, ['subclonal'])),
                    (posteriors.automaton_switches(3), two)):
        Q = au.delta.shape[0]
        q = np.array([[a, z, 0, 0] for a, z in runs], dtype=np.int32)
        P = np.exp(b.region_automaton_raw(r, 1, q, sym[:, None, :], au.delta[None], np.array([au.start]), orig)[0])
        for i, (a, z) in enumerate(runs):
            read = [n for n in range(z, a - 1, -1) if orig[n]]
            state = np.full(NS, au.start)
            for n in read:
                state = au.delta[state, sym[b.seg_class[n]][st[:, n]]]
            freq = np.bincount(state, minlength=Q) / NS
            tol = 5 * np.sqrt(P[i] * (1 - P[i]) / NS) + 1e-9
            print('run [%d, %d] Q %d: exact %s sampled %s' % (a, z, Q, np.array2string(P[i], precision=4), np.array2string(freq, precision=4)))
            informative += int(((P[i] > 0.01) & (P[i] < 0.99)).sum())
            assert (np.abs(freq - P[i]) <= tol).all(), (a, z, Q, freq, P[i])
    print('informative (run, column) entries: %d' % informative)
    assert informative >= 3
    _close(m)


def _padded(delta, start, rng):
    """Unreachable states up to Q = 16, with transitions of their own (into any state)."""
    nauto, Q, A = delta.shape
    out = rng.randint(0, 16, size=(nauto, 16, A)).astype(np.uint8)
    out[:, :Q] = delta
    return out, start


def test_bit_identity(hip, cases):
    """A (restart, query) result depends on neither the batch of queries, their order, nor on unreachable states that pad the
    automaton to Q = 16."""
    for grid in GRIDS[:2]:
        case = cases[grid]
        runs = case.queries()
        delta, start = automata(5, 2)
        sym = symbol_tables(case.b.cn_classes, 2)
        combos = [(0, 0), (1, 1), (2, 2), (2, 0)]
        full = case.final(runs, sym, delta, start, combos)[0]
        for i in range(len(runs)):
            assert np.array_equal(case.final(runs[i:i + 1], sym, delta, start, combos)[0, 0], full[i]), i
        assert np.array_equal(case.final(runs[::-1], sym, delta, start, combos)[0], full[::-1])
        assert np.array_equal(case.final(runs, sym, delta, start, combos[::-1])[0], full[:, ::-1])
        big, _ = _padded(delta, start, np.random.RandomState(8))
        wide = case.final(runs, sym, big, start, combos)[0]
        assert wide.shape[-1] == 16 and np.array_equal(wide[..., :5], full) and (wide[..., 5:] == -np.inf).all()
        # an automaton among 64, a symbol table among several
        many = np.concatenate([np.zeros((61, 5, 2), dtype=np.uint8), delta])
        assert np.array_equal(case.final(runs, sym, many, np.concatenate([np.zeros(61, dtype=np.int32), start]), [(si, ui + 61) for si, ui in combos])[0], full)


def test_restart_ranges_and_staging_chunks(hip):
    """Four restarts: a call over 0 .. 3 equals the single-restart calls bit for bit; a call with more queries than the 64 MiB
    staging buffer holds for four restarts of 16 columns runs in two chunks and repeats the short call's numbers."""
    from tests.test_hip_query_driver import _restart_set
    rs = _restart_set(4)
    try:
        b = rs.batch
        case = AutomatonCase(rs.models[0])
        runs = case.queries()
        delta, start = automata(16, 16)
        sym = symbol_tables(b.cn_classes, 16)
        combos = [(0, 0), (1, 1), (2, 2)]
        call = lambda r0, nr: case.final(runs, sym, delta, start, combos, r0=r0, nr=nr)
        full = call(0, 4)
        assert full.shape == (4, len(runs), 3, 16) and not np.isnan(full).any() and len(np.unique(full.reshape(4, -1), axis=0)) > 1
        for r in range(4):
            assert np.array_equal(call(r, 1)[0], full[r]), r
        assert np.array_equal(call(1, 2), full[1:3]) and np.array_equal(call(1, 3), full[1:])
        chunk = (64 << 20) // (4 * 16 * 8 + 16)
        short = [(a, z) for a, z in runs if z - a <= 1]
        base = np.array([[a, z, si, ui] for (a, z) in short for (si, ui) in combos], dtype=np.int32)
        reps = chunk // len(base) + 1
        assert reps * len(base) > chunk
        big = b.region_automaton_raw(0, 4, np.tile(base, (reps, 1)), sym, delta, start, case.constrain)
        small = b.region_automaton_raw(0, 4, base, sym, delta, start, case.constrain)
        assert np.array_equal(big.reshape(4, reps, len(base), 16), np.broadcast_to(small[:, None], (4, reps, len(base), 16)))
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
        case = AutomatonCase(m, batch=b, r=0)
        sym = symbol_tables(classes, 16)
        assert not np.array_equal(sym[0, 0], sym[1, 0]) and not np.array_equal(sym[0, 1], sym[1, 1])      # the symbol tables differ per class
        worst, _ = case.check(case.queries(), shapes=((16, 16),), tag='two classes')
        assert worst <= 1.
        # clone 1's total is >= 2 under class 1 and can be 0 under class 0: "some segment has clone 1 at total < 2" as a trap automaton.
        # (a kernel that took class 0's symbols everywhere would find that event in the odd segments too)
        low = posteriors.level_mask(classes, 'total', 1, 0, 1)
        assert low[0].any() and not low[1].any()
        trap = np.array([[[0, 1], [1, 1]]], dtype=np.uint8)
        odd = [(n, n) for n in range(1, N, 2)]
        even = [(n, n) for n in range(0, N, 2)]
        s1 = low.astype(np.int16)[:, None, :]
        assert (case.final(odd, s1, trap, np.array([0]), [(0, 0)], constrain=None)[0, :, 0, 1] == -np.inf).all()
        assert np.isfinite(case.final(even, s1, trap, np.array([0]), [(0, 0)], constrain=None)[0, :, 0, 1]).any()
    finally:
        b.close()


def test_mixed_transition_model(hip):
    """The snapshot of the last update_p_cn under another transition_model than the current one, both directions."""
    m = _fitted(hip, 40, 3, 4, seed=3)
    T0 = np.array(m.model.log_transmat)
    m.model.transition_model = 1
    assert np.array_equal(np.array(m.model.log_transmat), T0)            # the snapshot stays the model-0 one
    case = AutomatonCase(m)
    worst, _ = case.check(case.queries(), shapes=((16, 16), (5, 2)), tag='mixed model 0 -> 1')
    assert worst <= 1.
    m2 = _fitted(hip, 40, 3, 4, seed=3, transition_model=1)
    assert m2.model.transition_model == 1
    m2.model.transition_model = 0
    case2 = AutomatonCase(m2)
    assert not np.array_equal(np.array(m2.model.log_transmat), T0)
    worst, _ = case2.check(case2.queries(), shapes=((16, 16), (5, 2)), tag='mixed model 1 -> 0')
    assert worst <= 1.
    _close(m, m2)


def _inserted(hip):
    e = synthetic.make_experiment(60, num_clones=3, max_copy_number=4, num_chains=3, seed=7)
    e.breakpoints = H.add_shared_boundary_breakpoints(e)
    m, h, _ = H.make_model(hip, M=3, max_cn=4, experiment=e)
    H.attach(m, h)
    m.model.allele_likelihood_mask = np.zeros(m.model.num_segments, dtype=int)      # (events of intermediate probability)
    m.variational_update(); m.variational_update()
    return m


def test_inserted_segments(hip):
    """Two breakends on one boundary: the model inserts a zero-length segment there.  With constrain = seg_is_original the
    automaton does not read it; with constrain = NULL it does, and the count differs."""
    m = _inserted(hip)
    case = AutomatonCase(m)
    assert m.N1 > m.N and not case.constrain.all()
    dummy = int(np.flatnonzero(~case.constrain & (np.arange(m.N1) > 0) & (case.tel == 0))[0])
    assert case.constrain[dummy - 1] and case.constrain[dummy + 1]
    runs = [(dummy - 1, dummy + 1), (dummy, dummy), (dummy, dummy + 1), (dummy - 1, dummy), (dummy - 3, dummy + 2)]
    worst, _ = case.check(runs, shapes=((16, 16), (5, 2)), tag='inserted segment, not read')
    assert worst <= 1.
    worst, _ = case.check(runs, shapes=((5, 2),), constrain=None, tag='inserted segment, read')
    assert worst <= 1.
    # a counter of read segments (saturating at 3): the inserted one counts under NULL and does not under seg_is_original
    count = np.array([[[1, 1], [2, 2], [3, 3], [3, 3]]], dtype=np.uint8)
    sym = np.zeros(case.b.cn_classes.shape[:2], dtype=np.int16)[:, None, :]
    for constrain, want in ((case.constrain, [2, 0, 1, 1, 3]), (None, [3, 1, 2, 2, 3])):
        got = case.final(runs, sym, count, np.array([0]), [(0, 0)], constrain=constrain)[0, :, 0]
        assert np.array_equal(np.argmax(got, axis=-1), want) and (np.abs(got.max(axis=-1)) <= 6e-9).all() and ((got == -np.inf).sum(axis=-1) == 3).all(), (constrain, got)
    # the number of subclonal runs of the experiment pair around it, through event_runs: the twin on the model run, the inserted segment skipped
    i = int(m.seg_rev_remap[dummy - 1])
    assert m.seg_fwd_remap[i] == dummy - 1 and m.seg_fwd_remap[i + 1] == dummy + 1
    out = m.event_runs([(i, i + 1)], 'subclonal', bins=3)
    au = posteriors.automaton_runs(3)
    ev = posteriors.symbols_from(case.b.cn_classes, ['subclonal'])[case.b.seg_class]
    want = np.exp(automaton_twin.logfinal(case.twin, dummy - 1, dummy + 1, ev, au.delta, au.start, case.constrain)).reshape(3, 2).sum(axis=-1)
    assert out['num_events'].shape == (1, 3) and np.abs(out['num_events'][0] - want).max() <= 3e-9 and out['num_events'][0, 2] == 0
    _close(m)


def test_no_side_effects(hip):
    m1 = _fitted(hip, 50, 3, 4, seed=2)
    m2 = _fitted(hip, 50, 3, 4, seed=2)
    before = _model_state(m1)
    out = m1.event_runs([(0, 10), (5, 5), (3, 12)], 'loh')
    run = m1.event_run_of([(0, 10), (5, 5)], 'subclonal', 2)
    assert out['num_events'].shape == (3, 8) and out['p_any'].shape == (3,) and run['p_run'].shape == (2,) and run['p_run'][1] == 0
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
    delta, start = automata(5, 3)
    sym = symbol_tables(b.cn_classes, 3)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    ok = [[int(cs[0]), int(cs[0]) + 1, 0, 1]]
    with pytest.raises(ValueError, match='update_p_cn'):
        b.region_automaton_raw(r, 1, ok, sym, delta, start)
    assert bpmodel.last_error_restarts() == [r]
    with pytest.raises(ValueError, match='update_p_cn'):
        m.event_runs([(0, 3)], 'loh')
    m.variational_update()
    N = b.num_segments
    lib, handle = b._lib, b._handle
    dp, u8p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    assert b.region_automaton_raw(r, 1, ok, sym, delta, start).shape == (1, 1, 5)
    bad_delta = delta.copy(); bad_delta[-1, -1, -1] = 5
    bad_sym = sym.copy(); bad_sym[-1, -1, -1] = 3
    neg_sym = sym.copy(); neg_sym[0, 0, 0] = -1
    # (queries, symbols, delta, start, words of the message)
    bad = [(ok, sym, np.zeros((3, 17, 3), dtype=np.uint8), start, 'nauto'), (ok, sym[:, :, :], np.zeros((3, 5, 17), dtype=np.uint8), start, 'nauto'),
           (ok, sym, np.zeros((65, 5, 3), dtype=np.uint8), np.zeros(65, dtype=np.int32), 'nauto'), (ok, sym, np.zeros((3, 0, 3), dtype=np.uint8), start, 'nauto'),
           (ok, sym, np.zeros((3, 5, 0), dtype=np.uint8), start, 'nauto'),
           (ok, sym, bad_delta, start, 'transition or a start state'), (ok, sym, delta, np.array([0, 5, 0]), 'transition or a start state'),
           (ok, sym, delta, np.array([0, -1, 0]), 'transition or a start state'), (ok, bad_sym, delta, start, 'symbol is outside'), (ok, neg_sym, delta, start, 'symbol is outside'),
           (ok + [[0, 1, -1, 0]], sym, delta, start, 'symbol table index'), (ok + [[0, 1, 3, 0]], sym, delta, start, 'symbol table index'),
           (ok + [[0, 1, 0, -1]], sym, delta, start, 'automaton index'), (ok + [[0, 1, 0, 3]], sym, delta, start, 'automaton index'),
           (ok + [[3, 2, 0, 0]], sym, delta, start, 'first <= last'), (ok + [[int(ce[0]), int(ce[0]) + 1, 0, 0]], sym, delta, start, 'chain end'),
           (ok + [[0, N, 0, 0]], sym, delta, start, 'first <= last'), (ok + [[-1, 0, 0, 0]], sym, delta, start, 'first <= last')]
    for q, sy, dl, st, text in bad:
        # through the C entry point with an output buffer of its own: refused, and the buffer is untouched
        qa, args, _keep = b._region_args(q, None, sy, None)
        dl = np.ascontiguousarray(dl, dtype=np.uint8); st = np.ascontiguousarray(st, dtype=np.int32)
        dbuf = dl if dl.size else np.zeros(1, dtype=np.uint8)
        obuf = np.full((len(q), 16), 7.25)
        rc = lib.rmx_region_automaton(handle, r, 1, args[0], args[1], args[4], args[5], dl.shape[0], dl.shape[1], dl.shape[2], dbuf.ctypes.data_as(u8p),
                                      st.ctypes.data_as(i32p), None, obuf.ctypes.data_as(dp))
        assert rc == 5 and (obuf == 7.25).all(), (q, text, rc)
        with pytest.raises(ValueError, match='^bad argument: .*' + text):
            b.region_automaton_raw(r, 1, q, sy, dl, st)
        assert bpmodel.last_error_restarts() == []
    qa, args, _keep = b._region_args(ok, None, sym, None)
    obuf = np.full((2, 1, 5), 7.25)
    out = obuf.ctypes.data_as(dp)
    dl, st = delta.ctypes.data_as(u8p), start.ctypes.data_as(i32p)
    call = lambda r0=r, nr=1, nq=args[0], qp=args[1], nsym=args[4], sp=args[5], dlp=dl, stp=st, o=out: lib.rmx_region_automaton(
        handle, r0, nr, nq, qp, nsym, sp, 3, 5, 3, dlp, stp, None, o)
    for r0, nr in ((-1, 1), (0, 0), (0, 2)):
        assert call(r0=r0, nr=nr) == 5
    # nq < 1, NULL pointers (constrain excepted), nsym < 1
    assert call(nq=0) == 5 and call(qp=None) == 5 and call(sp=None) == 5 and call(nsym=0) == 5 and call(dlp=None) == 5 and call(stp=None) == 5 and call(o=None) == 5
    assert (obuf == 7.25).all()
    assert call() == 0 and not (obuf[0] == 7.25).any() and (obuf[1] == 7.25).all()
    with pytest.raises(ValueError):
        b.region_automaton_raw(r, 1, ok, sym, delta[0], start)
    with pytest.raises(ValueError):
        b.region_automaton_raw(r, 1, ok, sym, delta, start[:2])
    for call_, kw in ((m.event_runs, dict(event='loh', bins=9)), (m.event_runs, dict(event='gain')), (m.event_run_of, dict(event='loh', k=0))):
        with pytest.raises(ValueError):
            call_([(0, 3)], **kw)
    with pytest.raises(ValueError, match='two chains'):
        m.region_automaton([(0, 29)], posteriors.automaton_runs(2), posteriors.symbols_from(b.cn_classes, ['loh']))
    _close(m)


REGIONS = [(2, 7), (17, 17), (10, 30), (0, 39), (12, 13)]


def _examples(cn, chain):
    gain = posteriors.level_mask(cn, 'total', 'any', 3, 99)
    one_chain = [(2, 7), (17, 17), (13, int(np.flatnonzero(chain == chain[13])[-1]))]
    au = posteriors.automaton_switches(4)
    sym = posteriors.symbols_from(cn, [posteriors.level_mask(cn, 'total', 1, 0, 2), posteriors.level_mask(cn, 'total', 1, 3, 99)])
    return {'event_runs': [dict(regions=REGIONS, event='loh'), dict(regions=REGIONS, event=gain, bins=4)],
            'event_run_of': [dict(regions=REGIONS, event='subclonal', k=2), dict(regions=REGIONS, event=gain, k=3)],
            'region_automaton': [dict(regions=one_chain, automaton=au, symbols=sym), dict(regions=one_chain, automaton=au, symbols=sym, accept=[3, 4, 5, 6, 7, 8])]}


def _direct(name, b, r0, nr, m, a):
    maps = (m.seg_fwd_remap, m.seg_is_original, m.is_telomere)
    if name == 'event_runs':
        return posteriors.batch_event_runs(b, r0, nr, a['regions'], *maps, event=a['event'], bins=a.get('bins', 8))
    if name == 'event_run_of':
        return posteriors.batch_event_run_of(b, r0, nr, a['regions'], *maps, event=a['event'], k=a['k'])
    return posteriors.batch_region_automaton(b, r0, nr, a['regions'], *maps, automaton=a['automaton'], symbols=a['symbols'], accept=a.get('accept'))


def _same(a, b, where):
    assert isinstance(a, dict) and isinstance(b, dict) and list(a) == list(b), where
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == 'f'), (where, k)


def test_the_four_class_levels(hip):
    """Every level returns the numbers of the posteriors.batch_* function called directly, which asks the raw call; event_runs of a
    region in one chain is the count marginal of region_automaton with automaton_runs."""
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
        examples = _examples(b.cn_classes, chain)
        set_answers = {}
        for name, given_list in examples.items():
            for k, given in enumerate(given_list):
                want = _direct(name, b, 0, R, models[0], given)
                got = getattr(rs, name)(**given)
                _same(got, want, 'set: %s %d' % (name, k))
                set_answers[(name, k)] = got
                for r, m in enumerate(models):
                    one = dict((key, v[0]) for key, v in _direct(name, b, r, 1, m, given).items())
                    _same(getattr(m, name)(**given), one, 'model %d: %s %d' % (r, name, k))
        # against the raw call: a region inside one chain is one query
        fwd, m0 = np.asarray(models[0].seg_fwd_remap), models[0]
        au = posteriors.automaton_runs(8)
        q = np.array([[fwd[2], fwd[7], 0, 0]], dtype=np.int32)
        raw = b.region_automaton_raw(0, R, q, posteriors.symbols_from(b.cn_classes, ['loh'])[:, None, :], au.delta[None], np.array([0]), np.asarray(m0.seg_is_original))
        pmf = np.exp(raw[:, 0]).reshape(R, 8, 2).sum(axis=-1)
        assert np.abs(set_answers[('event_runs', 0)]['num_events'][:, 0] - pmf).max() <= 1e-15
        ra = set_answers[('region_automaton', 1)]
        assert np.abs(ra['final'].sum(axis=-1) - 1).max() <= 1e-7 and ra['p_accept'].shape == (R, 3) and (ra['p_accept'][:, 1] == 0).all()
    finally:
        rs.close()
    g = restarts.RestartGroups(e, ps, MAX_CN, groups=2, num_clones=3, quiet=True, seeds=list(range(R)), options={'fb_nv': 1})
    try:
        g.variational_update(2)
        g.synchronize()
        for name, given_list in examples.items():
            entry = queries.BY_NAME[name]
            for k, given in enumerate(given_list):
                parts = [getattr(part, name)(**given) for part in g.sets]
                got = getattr(g, name)(**given)
                _same(got, restarts._join(parts, shared=entry.shared), 'groups: %s %d' % (name, k))
                for key in got:
                    assert got[key].shape == set_answers[(name, k)][key].shape
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
