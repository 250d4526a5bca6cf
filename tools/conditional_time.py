"""Conditional posteriors given a region event (k_region_conditional) of all 16 restarts of the bench workload
(50 000 segments, 23 chains, one RestartSet) at 165 and 355 states, after one variational sweep, in one process.  The evidence is
an event over a 3-segment region in each of REGIONS chains, the window the region's whole chain.  Two events: 'loh', the one the
what-if question usually names -- under a normal clone of (1, 1) no state is LOH, the event cannot happen and every route ends at
once; it is kept as the measure of that case -- and 'total' (no change of the per-clone totals across the region), which can.
Three routes to the same numbers, the calls alternating, REPS times each, so that the spread between repeats stands beside a ratio:
  conditional   k_region_conditional: device time from rmx_profile_get, wall time of the raw call, and the floor from the sizes:
                three passes over the S^2 weights per evidence step, one per step right of the run and two per step left of it, and
                S Q weights per slot, all from L2;
  pattern       the exact route there was: one rmx_region_pattern query per (slot, feature) with the pieces (evidence, the feature's
                mask at the slot), for the features a mask can name (p_loh, p_hdel, p_subclonal), on SLOTS evenly spaced slots of each
                window outside the evidence run, scaled to all slots; it gives P(E and F_n), to be divided by P(E);
  samples       posterior samples per restart (sample_states, 64 at a time), those in E kept, the same three features averaged over
                them in numpy; with the share kept and the error against the exact route.
Usage: python tools/conditional_time.py [--samples K] [--reps N] [--regions R] [--slots S] [MAXCN ...]
(default 4096 samples, 3 repeats, 8 regions, 32 slots; 8 12: 165 and 355 states)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from remixt_amd import posteriors, sampling, synthetic
from remixt_amd.restarts import RestartSet

R, CHUNK = 16, 64
L2 = 34.5e12      # aggregate L2 rate
FEATURES = ('loh', 'hdel', 'subclonal')
args = sys.argv[1:]
opt = {'--samples': 4096, '--reps': 3, '--regions': 8, '--slots': 32}
while args and args[0] in opt:
    opt[args[0]] = int(args[1])
    args = args[2:]
K, REPS, REGIONS, SLOTS = opt['--samples'], opt['--reps'], opt['--regions'], opt['--slots']


def device_ms(b, fn, kernel):
    b.profile_reset(); b.profile_enable(1)
    t0 = time.perf_counter(); out = fn(); wall = time.perf_counter() - t0
    ms, n = b.profile().get(kernel, (0., 0)); b.profile_enable(0)
    return ms, n, wall * 1e3, out


def fmt(v):
    return ' '.join('%.3f' % x for x in v) + ' ms (median %.3f, spread %.1f %%)' % (np.median(v), 100. * (max(v) - min(v)) / max(np.median(v), 1e-12))


for mcn in [int(a) for a in args] or [8, 12]:
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=mcn, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, R, mcn)
    rs = RestartSet(e, ps, mcn, num_clones=3, quiet=True, seeds=list(range(R)))
    b, m = rs.batch, rs.models[0]
    rs.variational_update(1); b.synchronize()
    N, N1, S = len(e.l), b.num_segments, b.num_cn_states
    masks, labels = posteriors.event_tables(b.cn_classes)
    weights, layout = posteriors.feature_matrix(b.cn_classes)
    Q = layout['Q']
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    fwd = np.asarray(m.seg_fwd_remap, dtype=np.int64)
    constrain = np.ascontiguousarray(np.asarray(m.seg_is_original) != 0, dtype=np.uint8)
    # a 3-segment region in the middle of each of the first REGIONS chains (experiment segments)
    rev = np.full(N1, -1, dtype=np.int64); rev[fwd] = np.arange(N)
    regions = []
    for c in range(min(REGIONS, len(cs))):
        real = rev[cs[c]:ce[c] + 1]; real = real[real >= 0]
        k = int(real[len(real) // 2])
        regions.append((k, min(k + 2, int(real[-1]))))
    print('%d states, %d segments (%d in the model), %d chains, %d restarts, %d regions of 3 segments, chain windows, %d weight columns' % (
        S, N, N1, len(cs), R, len(regions), Q), flush=True)
    for event in ('loh', 'total'):
        mi, li = posteriors.parse_event(event)
        runs, windows, piece_region, _ = posteriors.conditional_queries(regions, 'chain', fwd, constrain, cs, ce)
        q = np.zeros((len(runs), 4), dtype=np.int32)
        q[:, :2], q[:, 2], q[:, 3] = runs, mi, li
        a_, b_, lo, hi = (x.astype(np.int64) for x in (q[:, 0], q[:, 1], windows[:, 0], windows[:, 1]))
        slots = int((hi - lo + 1).sum())
        floor = R * (((b_ - a_) * 3 + (hi - b_) + (a_ - lo) * 2).sum() * S * S + slots * S * Q) * 8 / L2 * 1e3
        cond = lambda: b.region_conditional_raw(0, R, q, windows, masks, labels, constrain, weights)
        # the pattern route on SLOTS slots per window, outside the run; three features per slot
        pieces, pq, where = [], [], []
        for i in range(len(q)):
            cand = np.arange(lo[i], hi[i] + 1)
            cand = cand[((cand < a_[i]) | (cand > b_[i])) & (constrain[cand] != 0)]
            for n in cand[np.linspace(0, len(cand) - 1, min(SLOTS, len(cand))).astype(int)]:
                for f in FEATURES:
                    ev, ft = [a_[i], b_[i], mi, li], [n, n, posteriors.MASK_NAMES.index(f), -1]
                    pq.append([len(pieces), 2, 0, 0]); pieces += [ft, ev] if n < a_[i] else [ev, ft]; where.append((i, n - lo[i], f))
        pq, pieces = np.array(pq, dtype=np.int32), np.array(pieces, dtype=np.int32)
        scale = slots / (len(pq) / len(FEATURES))
        pattern = lambda: b.region_pattern_raw(0, R, pq, pieces, masks, labels, constrain)
        cond(); pattern()
        tc, wc, tp, wp = [], [], [], []
        for rep in range(REPS):
            ms, nl, wall, (logp, out) = device_ms(b, cond, 'k_region_conditional'); tc.append(ms); wc.append(wall)
            ms, npl, wall, lj = device_ms(b, pattern, 'k_region_pattern'); tp.append(ms); wp.append(wall)
        possible = np.isfinite(logp)
        line = '  %s: %d (restart, query) pairs, %d slots each way, P(E) from %.3g to %.3g (%d pairs cannot happen): k_region_conditional %s over %d launches, ' \
               'call %.1f ms wall; floor (3 S^2 weights per evidence step, 1 right and 2 left of it, S Q per slot / 34.5 TB/s of L2) %.3f ms (x%.2f)' % (
                   event, len(q) * R, slots, np.exp(logp.min()), np.exp(logp.max()), (~possible).sum(), fmt(tc), nl, np.median(wc), floor,
                   np.median(tc) / floor)
        line += '; pattern route: %d queries on %d of %d slots: k_region_pattern %s over %d launches, call %.1f ms wall; scaled to every slot x%.1f: ' \
                '%.1f ms device; pattern / conditional x%.1f device, x%.1f wall' % (
                    len(pq) * R, len(pq) // len(FEATURES), slots, fmt(tp), npl, np.median(wp), scale, np.median(tp) * scale,
                    np.median(tp) * scale / max(np.median(tc), 1e-12), np.median(wp) * scale / max(np.median(wc), 1e-12))
        if possible.any():
            err = 0.
            for j, (i, k, f) in enumerate(where):
                ok = possible[:, i]
                err = max(err, np.abs(np.exp(lj[ok, j] - logp[ok, i]) - out[ok, i, k, layout[f]]).max())
            line += '; between the routes max |d P(F | E)| %.3e over %d (slot, feature) pairs' % (err, len(where))
        print(line, flush=True)
        # the sample route: K samples per restart, those in E kept
        lab_seg = None if li < 0 else labels[np.asarray(b.seg_class), li]                  # (N1, S)
        mask_seg = None if mi < 0 else masks[np.asarray(b.seg_class), mi] != 0
        feat_seg = np.stack([masks[np.asarray(b.seg_class), posteriors.MASK_NAMES.index(f)] != 0 for f in FEATURES])      # (3, N1, S)
        seeds = [sampling.restart_seed(0, i) for i in range(R)]
        b.sample_states(0, R, CHUNK, seeds)
        t_draw = t_count = 0.
        kept = np.zeros((R, len(q)))
        sums = [np.zeros((R, hi[i] - lo[i] + 1, len(FEATURES))) for i in range(len(q))]
        for k0 in range(0, K, CHUNK):
            t0 = time.perf_counter()
            st = b.sample_states(0, R, CHUNK, [s + k0 for s in seeds])      # (a fresh stream per chunk: the cost is what is measured)
            t1 = time.perf_counter()
            for i in range(len(q)):
                n = np.arange(a_[i], b_[i] + 1)
                inE = np.ones(st.shape[:2], dtype=bool)
                if mask_seg is not None:
                    nb = n[constrain[n] != 0]
                    inE &= mask_seg[nb[None, None], st[:, :, nb]].all(axis=2)
                if lab_seg is not None:
                    lb = lab_seg[n[None, None], st[:, :, n]]
                    inE &= (lb[:, :, 1:] == lb[:, :, :-1]).all(axis=2)
                kept[:, i] += inE.sum(axis=1)
                w = np.arange(lo[i], hi[i] + 1)
                sw = st[:, :, w]
                for f in range(len(FEATURES)):
                    sums[i][:, :, f] += (feat_seg[f][w[None, None], sw] & inE[:, :, None]).sum(axis=1)
            t_draw += t1 - t0; t_count += time.perf_counter() - t1
        line = '  %s, sample route, %d samples x %d restarts in chunks of %d: sample_states %.0f ms wall + filtering and averaging in numpy %.0f ms = %.0f ms; ' \
               'share of the samples in E: min %.3g, median %.3g' % (event, K, R, CHUNK, t_draw * 1e3, t_count * 1e3, (t_draw + t_count) * 1e3,
                                                                     (kept / K).min(), np.median(kept / K))
        if possible.any():
            errs = []
            for i in range(len(q)):
                ok = possible[:, i] & (kept[:, i] > 0)
                est = sums[i][ok] / kept[ok, i][:, None, None]
                exact = np.stack([out[ok, i, :hi[i] - lo[i] + 1, layout[f]] for f in FEATURES], axis=2)
                if ok.any():
                    errs.append(np.abs(est - exact).max())
            line += '; |sample estimate - exact| of the three features, max over slots %.3e (1 / sqrt(K P(E)) at the median share: %.3e); ' \
                    'sample route / conditional x%.0f wall' % (max(errs) if errs else np.nan, (K * max(np.median(kept / K), 1e-300)) ** -0.5,
                                                               (t_draw + t_count) * 1e3 / max(np.median(wc), 1e-12))
        print(line, flush=True)
    rs.close()
