"""Locus joints (k_locus_joint) of all 16 restarts of the bench workload (50 000 segments in 23 chains, one RestartSet) at 165 and
355 states, after one variational sweep, in one process, beside the route that gave the same numbers before: rmx_region_pattern
with bins^2 two-piece queries of 0/1 masks per pair, bins = 8.  Workloads, all with the tumour clones' highest total on both
sides (the table 'peak_total_any'):
  20 000 random pairs of one chain, 1 .. 64 segments apart;
  the breakpoints whose two breakends share a chain: the segment left of the first breakend against the one right of the second;
  46 arm-length pairs (the two ends of every 46th of the genome, where they share a chain);
  the dependence profile (window 64) of 1 000 anchors: one profile query per anchor for the left half and one pair query per
  right neighbour -- against the pattern route on the first PATTERN_ANCHORS anchors only (64 pattern queries per neighbour:
  the whole workload would be 8.2 million queries of 16 restarts), both reported per anchor.
k_locus_joint has no profile id, so both routes are timed the same way: HIP events on the batch's stream around the whole call
(rmx_timer_start / rmx_timer_stop: the launches of every chunk and the copies of queries and results between them) and wall
clock.  Per workload the routes alternate REPS times after a warm-up of each; medians and spreads are printed, and the largest
difference between the two routes in P and in log P (over the cells above e^-300 in both).  Beside them k_region_extremes on
the same runs with 16 columns, from its profile id, for the per-step comparison.
Usage: python tools/locus_joint_time.py [--reps N] [--anchors A] [--pairs P] [MAXCN ...]
(default 5 repeats, 1000 anchors, 20 000 random pairs; 8 12: 165 and 355 states)"""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from remixt_amd import posteriors, synthetic
from remixt_amd.restarts import RestartSet

R, BINS, WINDOW, PATTERN_ANCHORS = 16, 8, 64, 20
args = sys.argv[1:]
REPS, ANCHORS, NPAIRS = 5, 1000, 20000
while args and args[0] in ('--reps', '--anchors', '--pairs'):
    if args[0] == '--reps':
        REPS = int(args[1])
    elif args[0] == '--anchors':
        ANCHORS = int(args[1])
    else:
        NPAIRS = int(args[1])
    args = args[2:]


def timed(b, fn):
    b.synchronize()
    b.timer_start()
    t0 = time.perf_counter(); out = fn(); wall = time.perf_counter() - t0
    return b.timer_stop(), wall * 1e3, out


def fmt(v):
    return 'median %.3f ms, spread %.1f %%' % (np.median(v), 100. * (max(v) - min(v)) / np.median(v))


def pattern_route(b, pairs, masks):
    """The tables of model segment pairs a < t from rmx_region_pattern: BINS^2 queries of two one-segment pieces per pair."""
    i, j = np.divmod(np.arange(BINS * BINS), BINS)
    pieces = np.zeros((len(pairs), BINS * BINS, 2, 4), dtype=np.int32)
    pieces[:, :, 0, 0] = pieces[:, :, 0, 1] = pairs[:, None, 0]
    pieces[:, :, 1, 0] = pieces[:, :, 1, 1] = pairs[:, None, 1]
    pieces[:, :, 0, 2], pieces[:, :, 1, 2], pieces[:, :, :, 3] = i[None], BINS + j[None], -1
    q = np.zeros((len(pairs) * BINS * BINS, 4), dtype=np.int32)
    q[:, 0], q[:, 1] = 2 * np.arange(len(q)), 2
    pieces = pieces.reshape(-1, 4)
    return lambda: b.region_pattern_raw(0, R, q, pieces, masks, None, None).reshape(R, len(pairs), BINS, BINS)


def compare(new, old):
    with np.errstate(invalid='ignore', over='ignore'):
        dP = np.abs(np.exp(new) - np.exp(old)).max()
        both = (new > -300) & (old > -300)
        dF = np.abs(new - old)[both].max() if both.any() else 0.
    return 'largest difference between the routes: %.3e in P, %.3e in log P over %d cells above e^-300 in both (%d cells -inf in one route alone)' % (
        dP, dF, int(both.sum()), int(((new == -np.inf) != (old == -np.inf)).sum()))


for mcn in [int(a) for a in args] or [8, 12]:
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=mcn, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, R, mcn)
    rs = RestartSet(e, ps, mcn, num_clones=3, quiet=True, seeds=list(range(R)))
    b, m = rs.batch, rs.models[0]
    rs.variational_update(1); b.synchronize()
    N, N1, S = len(e.l), b.num_segments, b.num_cn_states
    levels, names = posteriors.locus_level_tables(b.cn_classes, BINS)
    lv = names.index('peak_total_any')
    ext_levels, ext_names = posteriors.level_tables(b.cn_classes, 16)
    masks = np.concatenate([levels[:, lv, None, :] == np.arange(BINS)[None, :, None]] * 2, axis=1).astype(np.uint8)
    fwd = np.asarray(m.seg_fwd_remap, dtype=np.int64)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    chain = np.searchsorted(ce, np.arange(N1), side='left')
    one_chain = lambda p: p[(chain[p[:, 0]] == chain[p[:, 1]]) & (p[:, 0] < p[:, 1])]
    rng = np.random.RandomState(0)
    first = rng.randint(0, N - 65, size=NPAIRS)
    near = one_chain(np.stack([fwd[first], fwd[first + rng.randint(1, 65, size=NPAIRS)]], axis=1))
    adj = posteriors.breakend_adjacencies(m.breakpoint_idx, m.num_breakpoints)
    adj = adj[(adj >= 0).all(axis=1)]
    ends = one_chain(np.stack([adj[:, 0], np.minimum(adj[:, 1] + 1, N1 - 1)], axis=1))
    edges = np.linspace(0, N, 47).astype(int)
    arms = one_chain(np.stack([fwd[edges[:-1]], fwd[edges[1:] - 1]], axis=1))
    print('%d states, %d segments (%d in the model), %d chains, %d restarts, %d x %d tables' % (S, N, N1, len(cs), R, BINS, BINS), flush=True)
    for name, pairs in (('%d random pairs 1-64 segments apart' % len(near), near), ('%d breakpoints with both breakends in one chain' % len(ends), ends),
                        ('%d arm-length pairs' % len(arms), arms)):
        pairs = pairs.astype(np.int32)
        q = np.concatenate([pairs, np.full((len(pairs), 2), lv, dtype=np.int32)], axis=1)
        steps = int((pairs[:, 1] - pairs[:, 0]).sum()) * R
        new = lambda: b.locus_joint_raw(0, R, q, levels, BINS, BINS, 0)
        old = pattern_route(b, pairs, masks)
        qe = np.concatenate([pairs, np.full((len(pairs), 1), -1, dtype=np.int32), np.full((len(pairs), 1), ext_names.index('peak_total_any'), dtype=np.int32)], axis=1)
        ext = lambda: b.region_extremes_raw(0, R, qe, None, ext_levels, None, 16)
        print('  %s: %s' % (name, compare(new(), old())), flush=True)
        ext()
        tn, wn, to, wo, te = [], [], [], [], []
        for rep in range(REPS):
            ms, wall, _ = timed(b, new); tn.append(ms); wn.append(wall)
            ms, wall, _ = timed(b, old); to.append(ms); wo.append(wall)
            b.profile_reset(); b.profile_enable(1)
            ext()
            te.append(b.profile().get('k_region_extremes', (0., 0))[0]); b.profile_enable(0)
        print('  %s: %d (restart, pair) walks, %d backward steps, longest %d' % (name, len(pairs) * R, steps, int((pairs[:, 1] - pairs[:, 0]).max())), flush=True)
        print('    rmx_locus_joint, one query per pair:          stream %s; wall %s; %.3f us per step' % (fmt(tn), fmt(wn), np.median(tn) * 1e3 / max(steps, 1)), flush=True)
        print('    rmx_region_pattern, %d queries per pair:       stream %s; wall %s; x%.2f of the locus call' % (
            BINS * BINS, fmt(to), fmt(wo), np.median(to) / np.median(tn)), flush=True)
        print('    k_region_extremes on the same runs, 16 columns: kernel %s; %.3f us per step' % (fmt(te), np.median(te) * 1e3 / max(steps, 1)), flush=True)
    # the dependence profile: model segments, the anchors' chains alone
    anchors = np.sort(rng.choice(N, size=ANCHORS, replace=False))
    segment = posteriors.locus_windows(anchors, WINDOW, fwd, cs, ce)
    T = fwd[anchors]
    Lm = fwd[np.where(segment[:, :WINDOW + 1] >= 0, segment[:, :WINDOW + 1], N).min(axis=1)]
    nslot = int((T - Lm).max()) + 1
    qprof = np.stack([Lm, T, np.full(ANCHORS, lv), np.full(ANCHORS, lv)], axis=1).astype(np.int32)
    right = [(i, k) for i in range(ANCHORS) for k in range(WINDOW + 1, 2 * WINDOW + 1) if segment[i, k] >= 0]
    qpair = np.array([[T[i], fwd[segment[i, k]], lv, lv] for i, k in right], dtype=np.int32)
    step = max(1, (256 << 20) // (R * nslot * BINS * BINS * 8))

    def profile_route(n_anchors):
        def run():
            out = [b.locus_joint_raw(0, R, qprof[a0:a0 + step], levels, BINS, BINS, nslot) for a0 in range(0, n_anchors, step)]
            sel = [k for k, (i, _) in enumerate(right) if i < n_anchors]
            return np.concatenate(out, axis=1), b.locus_joint_raw(0, R, qpair[sel], levels, BINS, BINS, 0)
        return run
    # the pattern route on the first PATTERN_ANCHORS anchors: every neighbour of the window as a pair
    sub = min(PATTERN_ANCHORS, ANCHORS)
    nb = [(i, k) for i in range(sub) for k in range(2 * WINDOW + 1) if segment[i, k] >= 0 and k != WINDOW]
    pp = np.array([sorted((T[i], fwd[segment[i, k]])) for i, k in nb], dtype=np.int32)
    old = pattern_route(b, pp, masks)
    prof, pair = profile_route(sub)()
    ref = old()
    at = dict((ik, x) for x, ik in enumerate(right))      # (right is ordered by anchor: the first anchors' pairs come first)
    got = np.stack([prof[:, i, T[i] - fwd[segment[i, k]]] if k < WINDOW else pair[:, at[(i, k)]] for i, k in nb], axis=1)
    print('  dependence profile, first %d anchors: %s' % (sub, compare(got, ref)), flush=True)
    tn, wn, ts, to, wo = [], [], [], [], []
    full, part = profile_route(ANCHORS), profile_route(sub)
    full()
    for rep in range(REPS):
        ms, wall, _ = timed(b, full); tn.append(ms); wn.append(wall)
        ms, wall, _ = timed(b, part); ts.append(ms)
        ms, wall, _ = timed(b, old); to.append(ms); wo.append(wall)
    print('  dependence profile, window %d, %d anchors (%d slots per profile query, %d right neighbours): rmx_locus_joint stream %s; wall %s; %.3f ms per anchor' % (
        WINDOW, ANCHORS, nslot, len(right), fmt(tn), fmt(wn), np.median(tn) / ANCHORS), flush=True)
    print('    the first %d anchors alone: rmx_locus_joint stream %s, %.3f ms per anchor; rmx_region_pattern, %d queries per neighbour, stream %s; wall %s; %.3f ms per anchor; x%.2f' % (
        sub, fmt(ts), np.median(ts) / sub, BINS * BINS, fmt(to), fmt(wo), np.median(to) / sub, np.median(to) / np.median(ts)), flush=True)
    rs.close()
